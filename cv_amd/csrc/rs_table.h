// rs_table.h — the pieces the stages that build or rewrite the CSR observation table (obs_start, obs, obs_counts,
// landmarks_out) share on the device: the tile of a scan, the flag of a check, the scan of the tile sums, the store of an
// observation, the walk of a row too long for one lane, the tail behind the filled rows.  rs_table_host.h is the host half.
// A stage still writes its own Call struct, its decisions (include/akz_*_math.h, the text its host build compiles too) and its
// kernels' bodies between these calls.
#pragma once
#include "akz_common.h"
#include "rs_table_host.h"

constexpr int kTblBlock = 256;
constexpr int kTblWaves = kTblBlock / 64;
constexpr int kTblItems = 4;                                 // rows per thread of a scan tile
constexpr uint32_t kTblTile = kTblBlock * kTblItems;         // RS_LT_TILE rows
static_assert(kTblTile == (uint32_t)RS_LT_TILE, "the tile size the header exports");

// a wave whose lanes saw something bad sets the word once.  Every lane of the wave calls it.
__device__ __forceinline__ void tbl_flag(uint32_t* word, int bad)
{
    if (__any(bad) && (threadIdx.x & 63u) == 0u) atomicOr(word, 1u);
}

// One step of a scan behind a running carry, over a workgroup of W waves: -> run + the values of the threads below this one;
// run moves on by the workgroup's total.  All threads call it.
template <int W = kTblWaves>
__device__ __forceinline__ uint32_t tbl_scan_step(uint32_t& run, uint32_t v, uint32_t* s_wave)
{
    uint32_t total;
    const uint32_t at = run + akz_block_exclusive<W>(v, s_wave, &total);
    run += total;
    return at;
}

// n values -> their exclusive prefix, 64 W at a time behind a running carry; -> the total.  ONE workgroup of W waves, all
// threads call it.  in == out scans in place.
template <int W>
__device__ __forceinline__ uint32_t tbl_scan(const uint32_t* in, uint32_t* out, uint32_t n, uint32_t* s_wave)
{
    uint32_t carry = 0u;
    for (uint32_t t0 = 0; t0 < n; t0 += 64u * W) {
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t at = tbl_scan_step<W>(carry, t < n ? in[t] : 0u, s_wave);
        if (t < n) out[t] = at;
    }
    return carry;
}
template <int W = kTblWaves>
__device__ __forceinline__ uint32_t tbl_scan_in_place(uint32_t* v, uint32_t n, uint32_t* s_wave)
{
    return tbl_scan<W>(v, v, n, s_wave);
}

// observation o is written at obs_out[at] as a member of row `key`: its landmark goes to landmarks_out [n_blocks][cap] where
// the observation names a feature of the table (atomicMin behind a fill of 0xFFFFFFFF: a feature listed twice gets its lowest key)
__device__ __forceinline__ void tbl_put(uint2* obs_out, uint32_t* landmarks_out, uint32_t n_blocks, uint32_t cap, uint32_t at, uint2 o, uint32_t key)
{
    obs_out[at] = o;
    if (o.x < n_blocks && o.y < cap) atomicMin(&landmarks_out[(size_t)o.x * cap + o.y], key);
}

// The rows too long for one lane are handed to the wave, one after another in lane order: f(src) runs once per lane whose
// `wide` is set, wave-uniformly; it fetches the row's bounds from lane src (__shfl) and strides the 64 lanes over the list.
// Every lane of the wave calls it.
template <typename F>
__device__ __forceinline__ void tbl_for_wide_rows(bool wide, F f)
{
    unsigned long long pending = __ballot(wide);
    while (pending) {
        const int src = __ffsll((long long)pending) - 1;
        pending &= pending - 1ull;
        f(src);
    }
}

// One 64-entry step of a wave's ordered append: -> pos + the keeping lanes below this one (the slot of a lane that keeps its
// entry); pos moves on by the lanes that keep.  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t tbl_wave_append(uint32_t& pos, bool keep, uint32_t lane)
{
    const unsigned long long m = __ballot(keep);
    const uint32_t at = pos + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    pos += (uint32_t)__popcll(m);
    return at;
}

// The rows behind the filled ones, one lane per row first_row + k <= lm_room: every start there is the total, every count 0.
// *rows and *total are words an earlier launch of the call left (a row below *rows is that launch's).  One kernel for every
// stage whose tail is no more than this; rs_landmark_table.hip defines it.
__global__ void k_tbl_tail(uint32_t* obs_start_out, uint32_t* obs_counts_out, uint32_t first_row, uint32_t lm_room, const uint32_t* rows,
                           const uint32_t* total);
