// rs_reconstruction_merge.hip — cv-sfm's loop closure between two reconstructions on gfx950: the landmark map of the bridging
// frame (cv-sfm/src/lib.rs:2159-2170), incorporate_reconstruction (lib.rs:1817-1887) over two CSR landmark tables, out of place,
// and normalize_reconstruction (lib.rs:2241-2283).  Integer data movement in the shape of rs_landmark_table.hip — validate,
// count, exclusive scan over tiles of RS_LT_TILE rows, scatter — and a handful of pose products; every decision and all the
// arithmetic is include/akz_reconstruction_merge_math.h, the text the CPU checker (tests/cpp/reconstruction_merge_host.c)
// compiles too — parity: host build == HIP, byte for byte.
//
// rs_merge_map_device is one workgroup:
//   k_mr_map          the feature -> final match table of the slot (the lowest match that names the feature), then an ordered
//                     compaction over the features (akz_block_scan): one entry per final match, in ascending feature order.
// rs_incorporate_reconstruction_device, in stream order:
//   k_ir_check        one lane per start, map entry and source view: do the starts of both tables ascend; the word of every block
//                     (a kept source view; a block the destination names: 256 workgroups stride over its observations behind an
//                     LDS bitmap); refs of the map.
//   k_ir_source_rows  one lane per source row: how many of its observations are kept, and what a kept one does to the call
//                     (a feature >= cap, a block the destination names).
//   k_ir_apply        one lane per map entry, on the complete refs and the call's verdict: applied (map_to[s] = d, map_from[d]
//                     = s; refs == 1 on both sides makes the lane their only writer) or demoted.
//   k_ir_tile_sums    first level of the scans: one lane per row gives its length, one workgroup per tile adds its tile — the
//                     destination's rows (old list + the kept list mapped to it) and the source's (is it a new row, how long).
//   k_ir_scan_sums    second level: ONE workgroup walks the tile sums kTblBlock at a time behind a running carry; the counts and
//                     the call's verdict.
//   k_ir_dest_rows    third pass over the destination: a workgroup scans its tile again, writes the starts and copies each row.
//   k_ir_source_out   third pass over the source: the key of every source landmark; the new rows' starts, lengths and lists.
//   k_tbl_tail        (rs_table.h) the starts and lengths of the empty rows up to lm_room.
//   k_ir_poses        the kept source views' poses times inverse(src_pose) * poses[bridge_block].
// A row whose lists hold more than kIrShortRow entries together is handed to its wave, which strides over it (a list can be as
// long as there are views) and places the kept observations by ballot: the position of every observation follows from the
// tables alone, so the bytes do not depend on the order anything arrives in.  The landmark of every observation written goes
// to d_landmarks_out where it is written (atomicMin behind a fill of 0xFFFFFFFF).  Nothing here waits on a value another
// workgroup has yet to write: the levels are separate launches; every loop is bounded by an argument or a checked count.
// rs_normalize_reconstruction_device is one workgroup of 256:
//   k_nr_normalize    the mean distance in include/akz_sum_order.h's order, then every view's pose and every constraint's
//                     translations.
// The three calls share the scratch rs_landmark_table.hip keeps in the context: they run on one stream, one after another.
#include "rs_table.h"
#include "../../include/akz_reconstruction_merge_math.h"

namespace {

constexpr uint32_t kIrShortRow = 64;                         // entries up to which one lane walks a row's lists
constexpr uint32_t kIrLdsBlocks = 65536;                     // blocks the LDS bitmap of k_ir_check holds (8 KB)
constexpr uint32_t kIrMarkGroups = 256;                      // workgroups of k_ir_check that mark the destination's blocks
static_assert(kTblBlock == AKZ_SUM_THREADS, "the workgroup akz_sum_order.h's T = 256 stands for");

static_assert(RS_IR_OK == AKZ_IR_OK && RS_IR_BAD_TABLE == AKZ_IR_BAD_TABLE && RS_IR_BAD_INDEX == AKZ_IR_BAD_INDEX &&
              RS_IR_SHARED_BLOCK == AKZ_IR_SHARED_BLOCK, "verdicts");
static_assert(RS_IR_C_ROWS == AKZ_IR_C_ROWS && RS_IR_C_OBSERVATIONS == AKZ_IR_C_OBSERVATIONS && RS_IR_C_APPLIED == AKZ_IR_C_APPLIED &&
              RS_IR_C_DEMOTED == AKZ_IR_C_DEMOTED && RS_IR_C_NEW_ROWS == AKZ_IR_C_NEW_ROWS && RS_IR_C_DROPPED == AKZ_IR_C_DROPPED &&
              RS_IR_COUNTS == AKZ_IR_COUNTS, "count words");
static_assert(RS_NR_OK == AKZ_NR_OK && RS_NR_NOT_NORMAL == AKZ_NR_NOT_NORMAL && RS_NR_BAD_INDEX == AKZ_NR_BAD_INDEX, "normalise verdicts");

// words of IrCall::info
enum { kIrBadDst = 0, kIrBadSrc = 1, kIrBadIndex = 2, kIrShared = 3, kIrApplied = 4, kIrDemoted = 5, kIrKept = 6, kIrDstTotal = 7, kIrRows = 8,
       kIrTotal = 9, kIrInfoWords = 16 };

// everything the kernels of one rs_incorporate_reconstruction_device call share, by value
struct IrCall {
    const uint32_t* dst_start;    // [n_dst + 1]
    const uint2* dst_obs;         // [n_dst_obs]
    const uint32_t* src_start;    // [n_src + 1]
    const uint2* src_obs;         // [n_src_obs]
    const uint2* map;             // [map_room]
    const uint32_t* map_count;    // [1]
    const double* src_pose;       // [12]
    const uint32_t* skip;         // [n_views] or null
    double* poses;                // [n_blocks][12]
    uint32_t* obs_start_out;      // [lm_room + 1]
    uint2* obs_out;               // [obs_room]
    uint32_t* counts_out;         // [AKZ_IR_COUNTS]
    uint32_t* landmarks_out;      // [n_blocks][cap]
    uint32_t* obs_counts_out;     // [lm_room]
    uint32_t* src_key_out;        // [n_src]
    uint32_t* call_verdict;       // [1]
    // scratch
    uint32_t* info;               // [kIrInfoWords]
    uint32_t* src_refs;           // [n_src] entries of the map that name the source landmark
    uint32_t* dst_refs;           // [n_dst] entries of the map that name the destination landmark
    uint32_t* kept_len;           // [n_src] kept observations of the source row
    uint32_t* bits;               // [n_blocks] AKZ_IR_BLOCK_*
    uint32_t* map_to;             // [n_src] d where an applied entry maps the source landmark, else none
    uint32_t* map_from;           // [n_dst] s where an applied entry maps to the destination landmark, else none
    uint32_t* tile_dst;           // [n_tiles_dst] a tile's observations, then its offset
    uint32_t* tile_rows;          // [n_tiles_src] a tile's new rows, then the new rows in front of it
    uint32_t* tile_obs;           // [n_tiles_src] a tile's new rows' observations, then those in front of it
    uint32_t* views;              // [n_views] src_blocks
    uint32_t cap, n_blocks, n_dst_obs, n_dst, n_src_obs, n_src, map_room, n_views, bridge_block, lm_room, n_tiles_dst, n_tiles_src;
};

__device__ __forceinline__ uint32_t ir_verdict(const IrCall& a)
{
    return akz_ir_verdict(a.info[kIrBadDst] != 0u || a.info[kIrBadSrc] != 0u, a.info[kIrBadIndex] != 0u, a.info[kIrShared] != 0u);
}

// info, src_refs, dst_refs, kept_len and bits are zero, map_to and map_from none in front of it
__global__ __launch_bounds__(kTblBlock) void k_ir_check(IrCall a)
{
    __shared__ uint32_t s_bits[kIrLdsBlocks / 32];
    const uint32_t i = blockIdx.x * kTblBlock + threadIdx.x;
    const int bad_dst = i <= a.n_dst && akz_lt_start_bad(a.dst_start, i, a.n_dst, a.n_dst_obs);
    const int bad_src = i <= a.n_src && akz_lt_start_bad(a.src_start, i, a.n_src, a.n_src_obs);
    tbl_flag(&a.info[kIrBadDst], bad_dst);
    tbl_flag(&a.info[kIrBadSrc], bad_src);
    if (i < a.n_views && !(a.skip && a.skip[i] != 0u)) atomicOr(&a.bits[a.views[i]], (uint32_t)AKZ_IR_BLOCK_KEPT);     // views[i] < n_blocks: the host
    // The blocks the destination names.  A table of 800 000 observations over 66 views would send 800 000 atomics to 66 words:
    // the first kIrMarkGroups workgroups stride over the observations, mark an LDS bitmap and hand on its set bits.
    const uint32_t fill = a.dst_start[a.n_dst] < a.n_dst_obs ? a.dst_start[a.n_dst] : a.n_dst_obs;
    const uint32_t groups = gridDim.x < kIrMarkGroups ? gridDim.x : kIrMarkGroups;
    if (blockIdx.x < groups) {                           // the same for every thread of the workgroup
        const bool in_lds = a.n_blocks <= kIrLdsBlocks;
        const uint32_t words = (a.n_blocks + 31u) / 32u;
        if (in_lds) {
            for (uint32_t w = threadIdx.x; w < words; w += kTblBlock) s_bits[w] = 0u;
            __syncthreads();
        }
        for (uint64_t k = (uint64_t)blockIdx.x * kTblBlock + threadIdx.x; k < fill; k += (uint64_t)groups * kTblBlock) {
            const uint32_t blk = a.dst_obs[k].x;
            if (blk >= a.n_blocks) continue;
            if (in_lds) atomicOr(&s_bits[blk >> 5], 1u << (blk & 31u));
            else atomicOr(&a.bits[blk], (uint32_t)AKZ_IR_BLOCK_DEST);
        }
        if (in_lds) {
            __syncthreads();
            for (uint32_t w = threadIdx.x; w < words; w += kTblBlock)
                for (uint32_t m = s_bits[w]; m; m &= m - 1u) atomicOr(&a.bits[32u * w + (uint32_t)__ffs((int)m) - 1u], (uint32_t)AKZ_IR_BLOCK_DEST);
        }
    }
    const uint32_t n_map = *a.map_count < a.map_room ? *a.map_count : a.map_room;
    if (i < n_map) {
        const uint2 e = a.map[i];
        if (e.x < a.n_src) atomicAdd(&a.src_refs[e.x], 1u);
        if (e.y < a.n_dst) atomicAdd(&a.dst_refs[e.y], 1u);
    }
}

__global__ __launch_bounds__(kTblBlock) void k_ir_source_rows(IrCall a)
{
    const uint32_t r = blockIdx.x * kTblBlock + threadIdx.x, lane = threadIdx.x & 63u;
    const bool on = r < a.n_src && a.info[kIrBadDst] == 0u && a.info[kIrBadSrc] == 0u;    // the starts ascend inside [0, n_src_obs]
    uint32_t kept = 0u;
    int bad_index = 0, shared = 0;
    if (on)
        for (uint32_t i = a.src_start[r], e = a.src_start[r + 1]; i < e; ++i) {
            const uint2 o = a.src_obs[i];
            if (!akz_ir_kept(a.bits, a.n_blocks, o.x)) continue;
            const uint32_t fault = akz_ir_kept_fault(a.bits, o.x, o.y, a.cap);
            bad_index |= fault == (uint32_t)AKZ_IR_BAD_INDEX;
            shared |= fault == (uint32_t)AKZ_IR_SHARED_BLOCK;
            ++kept;
        }
    if (on) a.kept_len[r] = kept;
    const uint32_t wave_kept = akz_wave_sum(kept);
    tbl_flag(&a.info[kIrBadIndex], bad_index);
    tbl_flag(&a.info[kIrShared], shared);
    if (wave_kept && lane == 0u) atomicAdd(&a.info[kIrKept], wave_kept);
}

__global__ __launch_bounds__(kTblBlock) void k_ir_apply(IrCall a)
{
    const uint32_t i = blockIdx.x * kTblBlock + threadIdx.x;
    const uint32_t n_map = *a.map_count < a.map_room ? *a.map_count : a.map_room;
    if (i >= n_map || ir_verdict(a) != (uint32_t)AKZ_IR_OK) return;
    const uint2 e = a.map[i];
    if (akz_ir_entry_applied(e.x, e.y, a.n_src, a.n_dst, a.src_refs, a.dst_refs)) {       // no other entry names e.x or e.y
        a.map_to[e.x] = e.y;
        a.map_from[e.y] = e.x;
        atomicAdd(&a.info[kIrApplied], 1u);
    } else {
        atomicAdd(&a.info[kIrDemoted], 1u);
    }
}

// is source row r < n_src a new row of the output, and how long
__device__ __forceinline__ bool ir_new_row(const IrCall& a, bool ok, uint32_t r, uint32_t* len)
{
    *len = a.kept_len[r];
    return ok && akz_ir_new_row(a.map_to[r], *len);
}

__global__ __launch_bounds__(kTblBlock) void k_ir_tile_sums(IrCall a)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    uint32_t tick = 0u, sum = 0u, rows = 0u;
    const bool dest = blockIdx.x < a.n_tiles_dst, ok = ir_verdict(a) == (uint32_t)AKZ_IR_OK;
    const uint32_t tile = dest ? blockIdx.x : blockIdx.x - a.n_tiles_dst;
#pragma unroll
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = tile * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;        // n + kTblTile < 2^32: the entry point
        if (dest && r < a.n_dst) {
            uint32_t len = 0u;
            if (a.info[kIrBadDst] == 0u) {
                const uint32_t m = a.map_from[r];                                        // m < n_src: k_ir_apply
                len = (a.dst_start[r + 1] - a.dst_start[r]) + (m != AKZ_LT_NONE ? a.kept_len[m] : 0u);
            }
            a.obs_counts_out[r] = len;
            sum += len;
        } else if (!dest && r < a.n_src) {
            uint32_t len;
            if (ir_new_row(a, ok, r, &len)) {
                sum += len;
                ++rows;
            }
        }
    }
    sum = akz_block_sum<kTblWaves>(s_cnt, tick, sum);
    rows = akz_block_sum<kTblWaves>(s_cnt, tick, rows);
    if (threadIdx.x == 0) {
        if (dest) a.tile_dst[tile] = sum;
        else {
            a.tile_obs[tile] = sum;
            a.tile_rows[tile] = rows;
        }
    }
}

__global__ __launch_bounds__(kTblBlock) void k_ir_scan_sums(IrCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t dst_total = tbl_scan_in_place(a.tile_dst, a.n_tiles_dst, s_wave);
    const uint32_t new_rows = tbl_scan_in_place(a.tile_rows, a.n_tiles_src, s_wave);
    const uint32_t new_obs = tbl_scan_in_place(a.tile_obs, a.n_tiles_src, s_wave);
    if (threadIdx.x == 0) {
        const uint32_t verdict = ir_verdict(a);
        const bool ok = verdict == (uint32_t)AKZ_IR_OK;                     // not ok: nothing was applied, no row is new
        a.info[kIrDstTotal] = dst_total;
        a.info[kIrRows] = a.n_dst + new_rows;
        a.info[kIrTotal] = dst_total + new_obs;
        a.counts_out[AKZ_IR_C_ROWS] = a.n_dst + new_rows;
        a.counts_out[AKZ_IR_C_OBSERVATIONS] = dst_total + new_obs;
        a.counts_out[AKZ_IR_C_APPLIED] = a.info[kIrApplied];
        a.counts_out[AKZ_IR_C_DEMOTED] = a.info[kIrDemoted];
        a.counts_out[AKZ_IR_C_NEW_ROWS] = new_rows;
        a.counts_out[AKZ_IR_C_DROPPED] = ok ? a.src_start[a.n_src] - a.info[kIrKept] : 0u;
        *a.call_verdict = verdict;
    }
}

// observation o is written at obs_out[at] as a member of row `key`
__device__ __forceinline__ void ir_put(const IrCall& a, uint32_t at, uint2 o, uint32_t key)
{
    tbl_put(a.obs_out, a.landmarks_out, a.n_blocks, a.cap, at, o, key);
}

// Every lane of the wave calls it.  on: this lane's row `key` is written from obs_out[at]: the destination's observations
// [ps, pe) as they are, then the kept ones of the source's [fs, fe), in their order.  Both ranges lie inside their tables (the
// starts were checked), the row's length was counted from the same ranges, and the sum of all lengths is at most n_dst_obs +
// n_src_obs <= obs_room.
__device__ __forceinline__ void ir_write_row(const IrCall& a, bool on, uint32_t key, uint32_t at, uint32_t ps, uint32_t pe, uint32_t fs, uint32_t fe)
{
    const uint32_t lane = threadIdx.x & 63u;
    const bool wide = on && (pe - ps) + (fe - fs) > kIrShortRow;
    if (on && !wide) {
        for (uint32_t i = ps; i < pe; ++i) ir_put(a, at++, a.dst_obs[i], key);
        for (uint32_t i = fs; i < fe; ++i) {
            const uint2 o = a.src_obs[i];
            if (akz_ir_kept(a.bits, a.n_blocks, o.x)) ir_put(a, at++, o, key);
        }
    }
    tbl_for_wide_rows(wide, [&](int src) {              // wave-uniform: every lane walks the same rows
        const uint32_t wkey = __shfl(key, src, 64), wat = __shfl(at, src, 64), wps = __shfl(ps, src, 64), wpe = __shfl(pe, src, 64);
        const uint32_t wfs = __shfl(fs, src, 64), wfe = __shfl(fe, src, 64);
        for (uint32_t i = wps + lane; i < wpe; i += 64u) ir_put(a, wat + (i - wps), a.dst_obs[i], wkey);
        uint32_t pos = wat + (wpe - wps);
        for (uint32_t q0 = wfs; q0 < wfe; q0 += 64u) {  // n_src_obs + 64 < 2^32: the entry point
            const uint32_t i = q0 + lane;
            const uint2 o = i < wfe ? a.src_obs[i] : make_uint2(AKZ_LT_NONE, AKZ_LT_NONE);
            const bool kept = i < wfe && akz_ir_kept(a.bits, a.n_blocks, o.x);
            const uint32_t slot = tbl_wave_append(pos, kept, lane);
            if (kept) ir_put(a, slot, o, wkey);
        }
    });
}

__global__ __launch_bounds__(kTblBlock) void k_ir_dest_rows(IrCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    uint32_t run = a.tile_dst[blockIdx.x];
#pragma unroll 1
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;
        const bool row = r < a.n_dst;
        const uint32_t len = row ? a.obs_counts_out[r] : 0u;
        const uint32_t at = tbl_scan_step(run, len, s_wave);
        if (row) a.obs_start_out[r] = at;
        uint32_t ps = 0u, pe = 0u, fs = 0u, fe = 0u;
        if (len != 0u) {                                  // never for a refused destination table: its lengths are 0
            ps = a.dst_start[r];
            pe = a.dst_start[r + 1];
            const uint32_t m = a.map_from[r];
            if (m != AKZ_LT_NONE) {
                fs = a.src_start[m];
                fe = a.src_start[m + 1];
            }
        }
        ir_write_row(a, len != 0u, r, at, ps, pe, fs, fe);
    }
}

__global__ __launch_bounds__(kTblBlock) void k_ir_source_out(IrCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const bool ok = ir_verdict(a) == (uint32_t)AKZ_IR_OK;
    uint32_t run_rows = a.n_dst + a.tile_rows[blockIdx.x], run_obs = a.info[kIrDstTotal] + a.tile_obs[blockIdx.x];
#pragma unroll 1
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;
        const bool row = r < a.n_src;
        uint32_t len = 0u;
        const bool fresh = row && ir_new_row(a, ok, r, &len);
        const uint32_t key = tbl_scan_step(run_rows, fresh ? 1u : 0u, s_wave), at = tbl_scan_step(run_obs, fresh ? len : 0u, s_wave);
        if (row) a.src_key_out[r] = !ok ? AKZ_LT_NONE : fresh ? key : a.map_to[r];
        if (fresh) {                                      // key < n_dst + n_src <= lm_room
            a.obs_start_out[key] = at;
            a.obs_counts_out[key] = len;
        }
        ir_write_row(a, fresh, key, at, 0u, 0u, fresh ? a.src_start[r] : 0u, fresh ? a.src_start[r + 1] : 0u);
    }
}

__global__ __launch_bounds__(kTblBlock) void k_ir_poses(IrCall a)
{
    if (ir_verdict(a) != (uint32_t)AKZ_IR_OK) return;
    double sp[12], bp[12], t[12];
    for (int k = 0; k < 12; ++k) {
        sp[k] = a.src_pose[k];
        bp[k] = a.poses[(size_t)12 * a.bridge_block + k];  // no view of the list is the bridging frame's block: nobody writes this row
    }
    akz_ir_transform(sp, bp, t);
    for (uint32_t v = blockIdx.x * kTblBlock + threadIdx.x; v < a.n_views; v += gridDim.x * kTblBlock) {
        if (a.skip && a.skip[v] != 0u) continue;
        double* row = a.poses + (size_t)12 * a.views[v];   // distinct blocks: this thread alone touches the row
        double p[12], o[12];
        for (int k = 0; k < 12; ++k) p[k] = row[k];
        akz_tvc_pose_mul(p, t, o);
        for (int k = 0; k < 12; ++k) row[k] = o[k];
    }
}

// ONE workgroup.  feat [cap] is scratch.
__global__ __launch_bounds__(kTblBlock) void k_mr_map(const uint32_t* __restrict__ matches, const uint32_t* __restrict__ nmatches,
                                                     const unsigned char* __restrict__ final_mask, const uint32_t* __restrict__ best, uint32_t n_world,
                                                     uint32_t n_dst, uint32_t cap, uint32_t f, const uint32_t* __restrict__ counts,
                                                     const uint32_t* __restrict__ src_landmarks, uint32_t bridge_block, uint32_t* feat, uint2* map,
                                                     uint32_t* map_count)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    const uint32_t count = counts[bridge_block], nm = nmatches[f];
    if (count > cap || nm > cap) {                        // the same for every thread
        if (threadIdx.x == 0) *map_count = 0u;
        return;
    }
    const uint32_t* src_lm = src_landmarks + (size_t)bridge_block * cap;
    for (uint32_t j = threadIdx.x; j < cap; j += kTblBlock) feat[j] = AKZ_LT_NONE;
    __threadfence_block();
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nm; i += kTblBlock) {
        const size_t at = (size_t)f * cap + i;
        uint32_t s, d;
        if (!final_mask[at]) continue;
        if (akz_mr_map_entry(matches[2 * at], matches[2 * at + 1], count, f, cap, n_world, n_dst, best, src_lm, &s, &d))
            atomicMin(&feat[matches[2 * at]], i);         // the feature is below count <= cap: akz_lt_match
    }
    __threadfence_block();
    __syncthreads();
    uint32_t base = 0u, tick = 0u;
    for (uint32_t j0 = 0; j0 < count; j0 += kTblBlock) {
        const uint32_t j = j0 + threadIdx.x;
        const uint32_t i = j < count ? feat[j] : AKZ_LT_NONE;
        uint32_t total;
        const uint32_t rank = akz_block_scan<kTblWaves>(s_cnt, tick, i != AKZ_LT_NONE, &total);
        if (i != AKZ_LT_NONE) {                           // base + rank < count <= cap: inside d_map
            const size_t at = (size_t)f * cap + i;
            uint32_t s, d;
            akz_mr_map_entry(matches[2 * at], matches[2 * at + 1], count, f, cap, n_world, n_dst, best, src_lm, &s, &d);
            map[base + rank] = make_uint2(s, d);
        }
        base += total;
    }
    if (threadIdx.x == 0) *map_count = base;
}

// ONE workgroup of AKZ_SUM_THREADS.
__global__ __launch_bounds__(kTblBlock) void k_nr_normalize(const uint32_t* __restrict__ views, uint32_t n_views, const uint32_t* __restrict__ counts,
                                                           const uint32_t* __restrict__ landmarks, uint32_t cap, uint32_t n_blocks,
                                                           const double* __restrict__ world, uint32_t n_world, double* poses, double* constraint_poses,
                                                           uint32_t n_constraints, double* stats, uint32_t* verdict)
{
    __shared__ double s_red[2][kTblWaves][1];
    __shared__ uint32_t s_cnt[2][kTblWaves];
    int bad = 0;
    for (uint32_t v = threadIdx.x; v < n_views; v += kTblBlock) bad |= views[v] >= n_blocks;
    bad = __syncthreads_or(bad);
    const uint32_t first = views[0];                      // n_views >= 1: the entry point
    if (!bad) bad = counts[first] > cap;
    if (bad) {                                            // the same for every thread
        if (threadIdx.x == 0) {
            stats[0] = 0.0;
            stats[1] = 0.0;
            *verdict = AKZ_NR_BAD_INDEX;
        }
        return;
    }
    const uint32_t count = counts[first];
    double pose[12];
    for (int k = 0; k < 12; ++k) pose[k] = poses[(size_t)12 * first + k];
    double part[1] = {0.0}, net[1];
    uint32_t n = 0u, tick = 0u;
    for (uint32_t j = threadIdx.x; j < count; j += kTblBlock) {
        const uint32_t lm = landmarks[(size_t)first * cap + j];
        double d;
        if (lm >= n_world || !akz_nr_distance(pose, world + 4 * (size_t)lm, &d)) continue;
        part[0] = part[0] + d;
        ++n;
    }
    akz_block_sum<kTblWaves, 1>(s_red, 0u, part, net);     // behind its barrier every thread holds the first view's old pose
    n = akz_block_sum<kTblWaves>(s_cnt, tick, n);
    const double mean = akz_nr_mean(net[0], n);
    const bool normal = akz_nr_is_normal(mean);
    if (threadIdx.x == 0) {
        stats[0] = mean;
        stats[1] = (double)n;
        *verdict = normal ? AKZ_NR_OK : AKZ_NR_NOT_NORMAL;
    }
    if (!normal) return;
    const double factor = 1.0 / mean;
    double inv[12];
    akz_tv_pose_inverse(pose, inv);
    for (uint32_t v = threadIdx.x; v < n_views; v += kTblBlock) {
        double* row = poses + (size_t)12 * views[v];      // distinct blocks: this thread alone touches the row
        double p[12], o[12];
        for (int k = 0; k < 12; ++k) p[k] = row[k];
        akz_nr_view(p, inv, factor, o);
        for (int k = 0; k < 12; ++k) row[k] = o[k];
    }
    for (size_t c = threadIdx.x; c < 2 * (size_t)n_constraints; c += kTblBlock) {
        double* p = constraint_poses + 12 * c;
        p[3] = p[3] * factor; p[7] = p[7] * factor; p[11] = p[11] * factor;
    }
}

}   // namespace

extern "C" int32_t rs_merge_map_device(rs_ctx* c, const void* d_matches, const void* d_nmatches, const void* d_final, const void* d_best,
                                       uint32_t n_world, uint32_t n_dst_landmarks, uint32_t cap_per_img, uint32_t slot, const void* d_counts,
                                       const void* d_src_landmarks, uint32_t n_blocks, uint32_t bridge_block, void* d_map, void* d_map_count,
                                       void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_matches || !d_nmatches || !d_final || !d_counts || !d_src_landmarks || !d_map || !d_map_count) return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || bridge_block >= n_blocks || slot > 65534u) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, akz_align_up(sizeof(uint32_t) * (size_t)cap_per_img, 256)));
        hipLaunchKernelGGL(k_mr_map, dim3(1), dim3(kTblBlock), 0, h.stream, (const uint32_t*)d_matches, (const uint32_t*)d_nmatches,
                           (const unsigned char*)d_final, (const uint32_t*)d_best, n_world, n_dst_landmarks, cap_per_img, slot,
                           (const uint32_t*)d_counts, (const uint32_t*)d_src_landmarks, bridge_block, (uint32_t*)ls->d_scratch, (uint2*)d_map,
                           (uint32_t*)d_map_count);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t rs_incorporate_reconstruction_device(rs_ctx* c, const void* d_dst_start, const void* d_dst_obs, uint32_t n_dst_obs,
                                                        uint32_t n_dst_landmarks, const void* d_src_start, const void* d_src_obs, uint32_t n_src_obs,
                                                        uint32_t n_src_landmarks, const void* d_map, const void* d_map_count, uint32_t map_room,
                                                        uint32_t cap_per_img, uint32_t n_blocks, const uint32_t* src_blocks, uint32_t n_src_views,
                                                        uint32_t bridge_block, const void* d_src_pose, const void* d_skip, uint32_t obs_room,
                                                        uint32_t lm_room, void* d_poses, void* d_obs_start_out, void* d_obs_out, void* d_counts_out,
                                                        void* d_landmarks_out, void* d_obs_counts_out, void* d_src_key_out, void* d_call_verdict,
                                                        void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_dst_start || (n_dst_obs != 0 && !d_dst_obs) || !d_src_start || (n_src_obs != 0 && !d_src_obs) || !d_map_count ||
            (map_room != 0 && !d_map) || !d_src_pose || !d_poses || !d_obs_start_out || !d_obs_out || !d_counts_out || !d_landmarks_out ||
            !d_obs_counts_out || !d_src_key_out || !d_call_verdict || (n_src_views != 0 && !src_blocks))
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || bridge_block >= n_blocks) return AKZ_E_INVALID;
        // row numbers of the last tile and observation numbers of the last wave step stay 32-bit
        if (n_dst_landmarks > 0xFFFFFFFFu - 2u * kTblTile || n_src_landmarks > 0xFFFFFFFFu - 2u * kTblTile || n_dst_obs > 0xFFFFFFFFu - 64u ||
            n_src_obs > 0xFFFFFFFFu - 64u || map_room > 0xFFFFFFFFu - kTblBlock)
            return AKZ_E_TOO_LARGE;
        // the rooms: no kernel can write past them (every observation written is one of an input table, every row one of theirs)
        if ((uint64_t)obs_room < (uint64_t)n_dst_obs + n_src_obs || (uint64_t)lm_room < (uint64_t)n_dst_landmarks + n_src_landmarks ||
            lm_room == 0xFFFFFFFFu)
            return AKZ_E_INVALID;
        std::vector<unsigned char> seen;
        if (!akz_distinct_blocks(src_blocks, n_src_views, n_blocks, &seen) || seen[bridge_block]) return AKZ_E_INVALID;
        // the input tables and the map are const: no output may lie over them
        const size_t w = sizeof(uint32_t);
        const void* in[5] = {d_dst_start, d_dst_obs, d_src_start, d_src_obs, d_map};
        const size_t in_bytes[5] = {w * ((size_t)n_dst_landmarks + 1), w * 2 * (size_t)n_dst_obs, w * ((size_t)n_src_landmarks + 1),
                                    w * 2 * (size_t)n_src_obs, w * 2 * (size_t)map_room};
        const void* out[6] = {d_obs_start_out, d_obs_out, d_obs_counts_out, d_landmarks_out, d_counts_out, d_src_key_out};
        const size_t out_bytes[6] = {w * ((size_t)lm_room + 1), w * 2 * (size_t)obs_room, w * (size_t)lm_room, w * (size_t)n_blocks * cap_per_img,
                                     w * AKZ_IR_COUNTS, w * (size_t)n_src_landmarks};
        if (!akz_outputs_clear_of_inputs(in, in_bytes, 5, out, out_bytes, 6)) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        const uint32_t nt_dst = (uint32_t)(((size_t)n_dst_landmarks + kTblTile - 1) / kTblTile), nt_src = (uint32_t)(((size_t)n_src_landmarks + kTblTile - 1) / kTblTile);
        const size_t src_bytes = w * ((size_t)n_src_landmarks + 1), dst_bytes = w * ((size_t)n_dst_landmarks + 1), ts_bytes = w * ((size_t)nt_src + 1);
        AkzScratchPlan plan;                                             // zero: info .. bits; none: map_to, map_from
        const size_t at_info = plan.take(w * kIrInfoWords), at_src_refs = plan.take(src_bytes), at_kept = plan.take(src_bytes);
        const size_t at_dst_refs = plan.take(dst_bytes), at_bits = plan.take(w * (size_t)n_blocks), at_to = plan.take(src_bytes), at_from = plan.take(dst_bytes);
        const size_t at_tile_dst = plan.take(w * ((size_t)nt_dst + 1)), at_tile_rows = plan.take(ts_bytes), at_tile_obs = plan.take(ts_bytes);
        const size_t at_views = plan.take(w * ((size_t)n_src_views + 1));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, plan.size()));
        char* base = (char*)ls->d_scratch;
        IrCall a;
        a.dst_start = (const uint32_t*)d_dst_start; a.dst_obs = (const uint2*)d_dst_obs; a.src_start = (const uint32_t*)d_src_start;
        a.src_obs = (const uint2*)d_src_obs; a.map = (const uint2*)d_map; a.map_count = (const uint32_t*)d_map_count;
        a.src_pose = (const double*)d_src_pose; a.skip = (const uint32_t*)d_skip; a.poses = (double*)d_poses;
        a.obs_start_out = (uint32_t*)d_obs_start_out; a.obs_out = (uint2*)d_obs_out; a.counts_out = (uint32_t*)d_counts_out;
        a.landmarks_out = (uint32_t*)d_landmarks_out; a.obs_counts_out = (uint32_t*)d_obs_counts_out; a.src_key_out = (uint32_t*)d_src_key_out;
        a.call_verdict = (uint32_t*)d_call_verdict;
        a.info = (uint32_t*)(base + at_info); a.src_refs = (uint32_t*)(base + at_src_refs); a.kept_len = (uint32_t*)(base + at_kept);
        a.dst_refs = (uint32_t*)(base + at_dst_refs); a.bits = (uint32_t*)(base + at_bits); a.map_to = (uint32_t*)(base + at_to);
        a.map_from = (uint32_t*)(base + at_from); a.tile_dst = (uint32_t*)(base + at_tile_dst); a.tile_rows = (uint32_t*)(base + at_tile_rows);
        a.tile_obs = (uint32_t*)(base + at_tile_obs); a.views = (uint32_t*)(base + at_views);
        a.cap = cap_per_img; a.n_blocks = n_blocks; a.n_dst_obs = n_dst_obs; a.n_dst = n_dst_landmarks; a.n_src_obs = n_src_obs;
        a.n_src = n_src_landmarks; a.map_room = map_room; a.n_views = n_src_views; a.bridge_block = bridge_block; a.lm_room = lm_room;
        a.n_tiles_dst = nt_dst; a.n_tiles_src = nt_src;
        AKZ_HIP(hipMemsetAsync(base + at_info, 0, at_to - at_info, h.stream));
        AKZ_HIP(hipMemsetAsync(base + at_to, 0xFF, at_tile_dst - at_to, h.stream));
        AKZ_HIP(hipMemsetAsync(d_landmarks_out, 0xFF, out_bytes[3], h.stream));
        if (n_src_views) AKZ_HIP(hipMemcpyAsync(a.views, src_blocks, w * n_src_views, hipMemcpyHostToDevice, h.stream));
        const dim3 block(kTblBlock);
        uint32_t widest = n_dst_landmarks + 1u;
        for (uint32_t v : {n_src_landmarks + 1u, map_room, n_src_views}) widest = v > widest ? v : widest;   // the observations are strided over
        hipLaunchKernelGGL(k_ir_check, dim3((widest + kTblBlock - 1) / kTblBlock), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_src_landmarks) {
            hipLaunchKernelGGL(k_ir_source_rows, dim3((n_src_landmarks + kTblBlock - 1) / kTblBlock), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        if (map_room) {
            hipLaunchKernelGGL(k_ir_apply, dim3((map_room + kTblBlock - 1) / kTblBlock), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        if (nt_dst + nt_src) {
            hipLaunchKernelGGL(k_ir_tile_sums, dim3(nt_dst + nt_src), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_ir_scan_sums, dim3(1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (nt_dst) {
            hipLaunchKernelGGL(k_ir_dest_rows, dim3(nt_dst), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        if (nt_src) {
            hipLaunchKernelGGL(k_ir_source_out, dim3(nt_src), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_tbl_tail, dim3((lm_room - n_dst_landmarks) / kTblBlock + 1), block, 0, h.stream, a.obs_start_out, a.obs_counts_out,
                           n_dst_landmarks, lm_room, (const uint32_t*)&a.info[kIrRows], (const uint32_t*)&a.info[kIrTotal]);   // a new row: k_ir_source_out
        AKZ_LAUNCH_CHECK();
        if (n_src_views) {
            const uint32_t grid = (n_src_views + kTblBlock - 1) / kTblBlock;
            hipLaunchKernelGGL(k_ir_poses, dim3(grid < 1024u ? grid : 1024u), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        return AKZ_OK;
    });
}

extern "C" int32_t rs_normalize_reconstruction_device(rs_ctx* c, const uint32_t* view_blocks, uint32_t n_views, const void* d_counts,
                                                      const void* d_landmarks, uint32_t cap_per_img, uint32_t n_blocks, const void* d_world,
                                                      uint32_t n_world, void* d_poses, void* d_constraint_poses, uint32_t n_constraints,
                                                      void* d_stats, void* d_verdict, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!view_blocks || n_views == 0 || !d_counts || !d_landmarks || (n_world != 0 && !d_world) || !d_poses || !d_stats || !d_verdict ||
            (n_constraints != 0 && !d_constraint_poses))
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0) return AKZ_E_INVALID;
        // two threads never write one row: the blocks inside the table are distinct (one outside it is RS_NR_BAD_INDEX's)
        std::vector<unsigned char> seen(n_blocks, 0);
        for (uint32_t v = 0; v < n_views; ++v) {
            if (view_blocks[v] >= n_blocks) continue;
            if (seen[view_blocks[v]]) return AKZ_E_INVALID;
            seen[view_blocks[v]] = 1;
        }
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, akz_align_up(sizeof(uint32_t) * (size_t)n_views, 256)));
        AKZ_HIP(hipMemcpyAsync(ls->d_scratch, view_blocks, sizeof(uint32_t) * (size_t)n_views, hipMemcpyHostToDevice, h.stream));
        hipLaunchKernelGGL(k_nr_normalize, dim3(1), dim3(kTblBlock), 0, h.stream, (const uint32_t*)ls->d_scratch, n_views, (const uint32_t*)d_counts,
                           (const uint32_t*)d_landmarks, cap_per_img, n_blocks, (const double*)d_world, n_world, (double*)d_poses,
                           (double*)d_constraint_poses, n_constraints, (double*)d_stats, (uint32_t*)d_verdict);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}
