// akz_keypoints.hip — gfx950 kernels for keypoint detection and description (SURVEY.md §8a rows
// A12a..A17).  -ffp-contract=off; every f32 expression follows the reference's order.
//
// Reference functions implemented here (paths relative to the rust-cv/cv checkout):
//   find_scale_space_extrema  candidate test   akaze/src/scale_space_extrema.rs:34-60    k_cand_count / k_cand_scatter
//   find_scale_space_extrema  serial pass      akaze/src/scale_space_extrema.rs:61-118   k_suppress
//   find_scale_space_extrema  upper-scale pass akaze/src/scale_space_extrema.rs:121-140  k_filter_upper
//   do_subpixel_refinement                     akaze/src/scale_space_extrema.rs:297-362  k_refine
//   compute_main_orientation + GAUSS25         akaze/src/scale_space_extrema.rs:162-288  k_refine
//   sort_unstable_by_key + truncate            akaze/src/lib.rs:326-327                  k_sort
//   extract_descriptors / get_mldb_descriptor  akaze/src/descriptors.rs:16-98            k_describe
//   mldb_fill_values / mldb_binary_comparisons akaze/src/descriptors.rs:102-202          k_describe
//
// Order-dependent parts keep the reference's order: candidates are compacted in (level, raster)
// order; the suppression cache is processed strictly sequentially per frame (parallel across the
// frames of the batch and, inside a frame, across the cache entries tested for one candidate);
// list compactions preserve order; the response sort is (response desc, index asc).
#include <algorithm>
#include <cmath>
#include <vector>

#include "akz_ctx.h"
#include "../../include/akz_portable_math.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Rust `f32 as usize`: truncate toward zero, negatives and NaN saturate to 0.
__device__ __forceinline__ unsigned sat_u32(float v) { return v > 0.0f ? (v >= 4294967040.0f ? 0xFFFFFFFFu : (unsigned)v) : 0u; }
// Rust `f32 as isize` (saturating); the values on this path are far inside the i32 range.
__device__ __forceinline__ int sat_i32(float v)
{
    if (v != v) return 0;
    if (v >= 2147483520.0f) return 2147483647;
    if (v <= -2147483648.0f) return (int)0x80000000;
    return (int)v;
}

struct LevelDesc {  // per-level constants for the keypoint kernels
    const float* Ldet;
    const float* Lt;
    const float2* Lxy;  // {Lx, Ly} interleaved
    int w, h;
    size_t fs;        // frame stride (pixels)
    uint32_t octave;
    float kp_size;    // (esigma * derivative_factor) as f32
    uint32_t row_off; // this level's first word in a frame's row-start table (k_cand_rows): h + 1 words per level
};
constexpr int kMaxLevels = kAkzMaxLevels;
struct LevelTable {
    LevelDesc L[kMaxLevels];
    int n;
    uint32_t rows_total;   // words of a frame's row-start table
};

// A12a (candidate test + border test) is fused into the second-order derivative kernel and followed by a
// per-level raster sort: k_deriv_second_cand / k_cand_sort in akz_scale_space.hip.

// ---------------------------------------------------------------------------------------------
// A12b: the order-dependent suppression pass (scale_space_extrema.rs:61-118).  ONE WAVE per frame, no
// workgroup barriers: the pass is a strict sequence over the frame's candidates, so the parallelism is
// (a) across the frames of the batch and (b) across the cache entries tested for one candidate.
//
// The reference scans the whole cache for the FIRST entry (in cache order) whose class_id is the
// candidate's level or the one below and that lies within the candidate's size.  Only entries of those
// two classes can match, so the wave keeps them — in cache order — in an LDS "active list" (rebuilt at
// each level change); pushes append to it and in-place replacements update it in place, so its order
// always equals cache order.  The list is cut into chunks of 64 entries (one per lane) and every chunk
// carries a conservative [ymin, ymax] of its entries (held in registers, only ever widened between rebuilds).  Candidates
// arrive in raster order, so the entries that can lie within `size` of one are confined to a few chunks:
// lane l tests chunk l's bounds, the ballot lists the chunks worth scanning, and they are scanned in
// ascending order until the first hit — the same entry the reference's linear scan finds.  The full
// cache goes to HBM in slot order for the second pass.
constexpr int kActCap = 8192;            // active-list capacity (entries of two adjacent classes)
static_assert(kActCap / 64 == 128, "chunk bounds are held two per lane");
struct ActEntry {   // 16 B
    float x, y;     // full-resolution coordinates (with the +0.5(ratio-1) offset, as cached)
    float resp;
    uint32_t slot_cls;  // slot (24 bits) | class (8 bits)
};

__device__ __forceinline__ float rl_f(float v, uint32_t l)
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), (int)l));
}
__device__ __forceinline__ uint32_t rl_u(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }

__global__ __launch_bounds__(64) void k_suppress(LevelTable T, const uint32_t* __restrict__ ncand,
                                                 const uint2* __restrict__ cand, uint32_t max_cand,
                                                 DevKp* __restrict__ cache, uint32_t max_kp,
                                                 uint32_t* __restrict__ ncache, uint32_t* __restrict__ err,
                                                 const uint32_t* __restrict__ only_flagged,
                                                 uint32_t* __restrict__ lvl_slot, uint32_t* __restrict__ big_flag)
{
    if (only_flagged && !only_flagged[blockIdx.x]) return;   // the parallel path (k_sup_*) did this frame
    // LDS: the active list only.  A single wave executes its DS instructions in order, so a ds_write by
    // lane 0 is seen by every later ds_read of the wave without any barrier.  The wave is issue-bound
    // (one dependent instruction stream), so the per-candidate path is kept as short as possible:
    // everything that does not depend on the cache (the border test) was done in k_cand_scatter.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    ActEntry* act = reinterpret_cast<ActEntry*>(smem);
    const int frame = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint2* cd = cand + (size_t)frame * kAkzMaxLevels * max_cand;
    DevKp* ch = cache + (size_t)frame * max_kp;
    uint32_t nact = 0, nslots = 0;  // wave-uniform
    bool overflowed = false;        // wave-uniform: a list ran out of room (the call then fails with AKZ_E_INTERNAL)
    // chunk bounds live in registers: lane l holds [ymin, ymax] of chunks l and l + 64
    float bmin0 = 3.0e38f, bmax0 = -3.0e38f, bmin1 = 3.0e38f, bmax1 = -3.0e38f;
    for (int e = 0; e < T.n; ++e) {
        const LevelDesc& L = T.L[e];
        if (lane == 0) lvl_slot[(size_t)frame * (kMaxLevels + 1) + e] = nslots;   // first slot pushed at level e
        // ---- level change: keep only class e-1 entries (class e-2 can no longer match), in order ----
        {
            uint32_t kept = 0;
            for (uint32_t b0 = 0; b0 < nact; b0 += 64) {
                uint32_t i = b0 + lane;
                float4 en = make_float4(0.f, 0.f, 0.f, 0.f);
                bool keep = false;
                if (i < nact) {
                    en = *reinterpret_cast<const float4*>(&act[i]);
                    keep = (int)(__float_as_uint(en.w) & 0xFFu) == e - 1;
                }
                unsigned long long bal = __ballot(keep);
                // reads of chunk b0 are complete (values are in registers) before the in-order writes below
                if (keep) *reinterpret_cast<float4*>(&act[kept + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))]) = en;
                kept += (uint32_t)__popcll(bal);
            }
            nact = kept;
            bmin0 = bmin1 = 3.0e38f;
            bmax0 = bmax1 = -3.0e38f;
            for (uint32_t b0 = 0; b0 < nact; b0 += 64) {
                uint32_t i = b0 + lane;
                float y = i < nact ? act[i].y : 0.0f;
                float lo = i < nact ? y : 3.0e38f, hi = i < nact ? y : -3.0e38f;
                for (int off = 32; off > 0; off >>= 1) {
                    lo = fminf(lo, __shfl_xor(lo, off));
                    hi = fmaxf(hi, __shfl_xor(hi, off));
                }
                uint32_t ck = b0 >> 6;
                if (lane == (ck & 63u)) {
                    if (ck < 64u) { bmin0 = lo; bmax0 = hi; }
                    else { bmin1 = lo; bmax1 = hi; }
                }
            }
        }
        const float ratio = ldexpf(1.0f, (int)L.octave);
        const float half_off = 0.5f * (ratio - 1.0f);
        const float size = L.kp_size;
        const float size2 = size * size;
        const float margin = size * 1.001f + 0.01f;  // conservative: |dy| > margin  =>  dist > size^2
        // this level's raster-sorted candidates (overflow beyond the capacity was flagged by the producer)
        const uint32_t c_begin = (uint32_t)e * max_cand;
        const uint32_t c_end = c_begin + min(ncand[(size_t)frame * kAkzMaxLevels + e], max_cand);
        for (uint32_t cb = c_begin; cb < c_end; cb += 64) {
            // one coalesced load of the next 64 candidates, then broadcast lane by lane
            uint2 mine = (cb + lane < c_end) ? cd[cb + lane] : make_uint2(0u, 0u);
            const uint32_t cnt = min(64u, c_end - cb);
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t cxy = rl_u(mine.x, t);
                const float resp = fabsf(__uint_as_float(rl_u(mine.y, t)));
                const float px = (float)(cxy & 0xFFFFu), py = (float)(cxy >> 16);
                const float fx = px * ratio, fy = py * ratio;
                // which chunks can hold an entry within `size` of the candidate?
                unsigned long long qm = __ballot(fy >= bmin0 - margin && fy <= bmax0 + margin);
                unsigned long long q1 = 0ull;
                if (nact > 4096u) q1 = __ballot(fy >= bmin1 - margin && fy <= bmax1 + margin);  // rare: > 64 chunks
                bool found = false;
                uint32_t first = 0u;
                float first_resp = 0.f;
                uint32_t first_sc = 0u;
                uint32_t kbase = 0u;
                for (;;) {
                    while (qm) {
                        uint32_t kk = kbase + (uint32_t)__ffsll((long long)qm) - 1u;
                        qm &= qm - 1ull;
                        uint32_t i = kk * 64u + lane;
                        ActEntry en = act[i < nact ? i : 0u];
                        float dx = fx - en.x, dy = fy - en.y;
                        unsigned long long hb = __ballot(i < nact && dx * dx + dy * dy <= size2);
                        if (hb) {
                            uint32_t hl = (uint32_t)__ffsll((long long)hb) - 1u;
                            found = true;
                            first = kk * 64u + hl;
                            first_resp = rl_f(en.resp, hl);
                            first_sc = rl_u(en.slot_cls, hl);
                            break;
                        }
                    }
                    if (found || q1 == 0ull) break;
                    qm = q1;  // the chunks 64..127, visited only when chunks 0..63 had no hit
                    q1 = 0ull;
                    kbase = 64u;
                }
                // decision (wave-uniform values): scale_space_extrema.rs:72-116; the border test already passed
                bool is_repeated = found && resp > first_resp;
                if (found && !is_repeated) continue;  // is_extremum = false
                uint32_t ai, slot;
                if (!is_repeated) {
                    ai = nact;
                    slot = nslots;
                    if (slot < max_kp && slot < (1u << 24) && ai >= (uint32_t)kActCap && big_flag) {
                        // more entries of two adjacent classes than the LDS list holds: the frame starts over in
                        // k_suppress_big, whose list lives in global memory (the reference's Vec has no limit)
                        if (lane == 0) big_flag[frame] = 1u;
                        return;
                    }
                    if (!(slot < max_kp && ai < (uint32_t)kActCap && slot < (1u << 24))) {
                        if (lane == 0) *err = 2u;
                        overflowed = true;
                        continue;
                    }
                    nact = ai + 1;
                    nslots = slot + 1;
                } else {
                    ai = first;
                    slot = first_sc >> 8;
                }
                // keypoint.point = p * ratio + 0.5 * (ratio - 1)  (:106-109)
                const float kx = fx + half_off, ky = fy + half_off;
                if (lane == 0) {
                    DevKp kp = {kx, ky, resp, size, __uint_as_float(cb + t - c_begin), L.octave, (uint32_t)e};   // angle <- index in level
                    ch[slot] = kp;
                    ActEntry w = {kx, ky, resp, (slot << 8) | (uint32_t)e};
                    act[ai] = w;
                }
                // widen (or start) the bounds of chunk ai/64 in the lane that owns it
                const uint32_t ck = ai >> 6;
                const bool fresh = !is_repeated && (ai & 63u) == 0u;
                if (lane == (ck & 63u)) {
                    if (ck < 64u) {
                        bmin0 = fresh ? ky : fminf(bmin0, ky);
                        bmax0 = fresh ? ky : fmaxf(bmax0, ky);
                    } else {
                        bmin1 = fresh ? ky : fminf(bmin1, ky);
                        bmax1 = fresh ? ky : fmaxf(bmax1, ky);
                    }
                }
            }
        }
    }
    if (lane == 0) {
        ncache[frame] = overflowed ? max_kp + 1u : nslots;   // (> max_kp = "did not fit": akz_last_overflow; readers clip)
        lvl_slot[(size_t)frame * (kMaxLevels + 1) + T.n] = nslots;
    }
}

// The same pass for a frame whose active list outgrew the LDS (more than 8 192 entries of two adjacent classes: only a
// context created for more than 8 192 keypoints per frame can get there, and only on frames the parallel pass handed
// back).  The reference's cache is a Vec: it has no such limit, so neither may the library (round-3 verdict: the last
// refusal on the extraction path).  Same walk, same decisions; what changes is where things live:
//   * the active list in global memory (`act`, max_kp entries per frame).  One wave reads what it wrote itself: every store is an agent-scope store followed by
//     s_waitcnt vmcnt(0) (it has reached the L2), every load an agent-scope load (it comes from the L2, not from a stale
//     L1 line);
//   * the chunk bounds in LDS (up to 4 096 chunks), tested 64 chunks at a time.
// Slow (a global round trip per replaced or pushed entry) and rare; it exists so that no input the reference handles ends
// in AKZ_E_INTERNAL.
constexpr int kBigChunks = (int)(kAkzMaxKeypoints / 64);
__device__ __forceinline__ ActEntry act_load(const ActEntry* p)
{
    const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
    const unsigned long long a = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long b = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ActEntry e;
    e.x = __uint_as_float((uint32_t)a);
    e.y = __uint_as_float((uint32_t)(a >> 32));
    e.resp = __uint_as_float((uint32_t)b);
    e.slot_cls = (uint32_t)(b >> 32);
    return e;
}
__device__ __forceinline__ void act_store(ActEntry* p, const ActEntry& e)
{
    unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
    __hip_atomic_store(q, (unsigned long long)__float_as_uint(e.x) | ((unsigned long long)__float_as_uint(e.y) << 32), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, (unsigned long long)__float_as_uint(e.resp) | ((unsigned long long)e.slot_cls << 32), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void act_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__global__ __launch_bounds__(64) void k_suppress_big(LevelTable T, const uint32_t* __restrict__ ncand, const uint2* __restrict__ cand,
                                                     uint32_t max_cand, DevKp* __restrict__ cache, uint32_t max_kp,
                                                     uint32_t* __restrict__ ncache, uint32_t* __restrict__ err,
                                                     const uint32_t* __restrict__ big_flag, uint32_t* __restrict__ lvl_slot,
                                                     ActEntry* __restrict__ act_all, uint32_t act_stride)
{
    if (!big_flag[blockIdx.x]) return;
    __shared__ float s_bmin[kBigChunks], s_bmax[kBigChunks];
    const int frame = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint2* cd = cand + (size_t)frame * kAkzMaxLevels * max_cand;
    DevKp* ch = cache + (size_t)frame * max_kp;
    ActEntry* act = act_all + (size_t)frame * act_stride;
    uint32_t nact = 0, nslots = 0;
    bool overflowed = false;
    for (int e = 0; e < T.n; ++e) {
        const LevelDesc& L = T.L[e];
        if (lane == 0) lvl_slot[(size_t)frame * (kMaxLevels + 1) + e] = nslots;
        {
            // level change: class e - 1 stays, in order (a chunk is read into registers before anything of it is rewritten,
            // and the kept entries only ever move towards the front)
            uint32_t kept = 0;
            for (uint32_t b0 = 0; b0 < nact; b0 += 64) {
                const uint32_t i = b0 + lane;
                ActEntry en = {0.f, 0.f, 0.f, 0u};
                bool keep = false;
                if (i < nact) {
                    en = act_load(&act[i]);
                    keep = (int)(en.slot_cls & 0xFFu) == e - 1;
                }
                const unsigned long long bal = __ballot(keep);
                if (keep) act_store(&act[kept + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))], en);
                act_stores_done();
                kept += (uint32_t)__popcll(bal);
            }
            nact = kept;
            for (uint32_t b0 = 0; b0 < nact; b0 += 64) {
                const uint32_t i = b0 + lane;
                const float y = i < nact ? act_load(&act[i]).y : 0.0f;
                float lo = i < nact ? y : 3.0e38f, hi = i < nact ? y : -3.0e38f;
                for (int off = 32; off > 0; off >>= 1) {
                    lo = fminf(lo, __shfl_xor(lo, off));
                    hi = fmaxf(hi, __shfl_xor(hi, off));
                }
                if (lane == 0) {
                    s_bmin[b0 >> 6] = lo;
                    s_bmax[b0 >> 6] = hi;
                }
            }
        }
        const float ratio = ldexpf(1.0f, (int)L.octave);
        const float half_off = 0.5f * (ratio - 1.0f);
        const float size = L.kp_size;
        const float size2 = size * size;
        const float margin = size * 1.001f + 0.01f;
        const uint32_t c_begin = (uint32_t)e * max_cand;
        const uint32_t c_end = c_begin + min(ncand[(size_t)frame * kAkzMaxLevels + e], max_cand);
        for (uint32_t cb = c_begin; cb < c_end; cb += 64) {
            const uint2 mine = (cb + lane < c_end) ? cd[cb + lane] : make_uint2(0u, 0u);
            const uint32_t cnt = min(64u, c_end - cb);
            for (uint32_t t = 0; t < cnt; ++t) {
                const uint32_t cxy = rl_u(mine.x, t);
                const float resp = fabsf(__uint_as_float(rl_u(mine.y, t)));
                const float px = (float)(cxy & 0xFFFFu), py = (float)(cxy >> 16);
                const float fx = px * ratio, fy = py * ratio;
                bool found = false;
                uint32_t first = 0u, first_sc = 0u;
                float first_resp = 0.f;
                const uint32_t nchunks = (nact + 63u) >> 6;
                for (uint32_t g = 0; g < nchunks && !found; g += 64) {
                    const uint32_t ck = g + lane;
                    unsigned long long qm = __ballot(ck < nchunks && fy >= s_bmin[ck < nchunks ? ck : 0u] - margin &&
                                                     fy <= s_bmax[ck < nchunks ? ck : 0u] + margin);
                    while (qm) {
                        const uint32_t kk = g + (uint32_t)__ffsll((long long)qm) - 1u;
                        qm &= qm - 1ull;
                        const uint32_t i = kk * 64u + lane;
                        const ActEntry en = act_load(&act[i < nact ? i : 0u]);
                        const float dx = fx - en.x, dy = fy - en.y;
                        const unsigned long long hb = __ballot(i < nact && dx * dx + dy * dy <= size2);
                        if (hb) {
                            const uint32_t hl = (uint32_t)__ffsll((long long)hb) - 1u;
                            found = true;
                            first = kk * 64u + hl;
                            first_resp = rl_f(en.resp, hl);
                            first_sc = rl_u(en.slot_cls, hl);
                            break;
                        }
                    }
                }
                const bool is_repeated = found && resp > first_resp;
                if (found && !is_repeated) continue;
                uint32_t ai, slot;
                if (!is_repeated) {
                    ai = nact;
                    slot = nslots;
                    if (!(slot < max_kp && ai < act_stride && slot < (1u << 24))) {
                        if (lane == 0) *err = 2u;
                        overflowed = true;
                        continue;
                    }
                    nact = ai + 1;
                    nslots = slot + 1;
                } else {
                    ai = first;
                    slot = first_sc >> 8;
                }
                const float kx = fx + half_off, ky = fy + half_off;
                if (lane == 0) {
                    DevKp kp = {kx, ky, resp, size, __uint_as_float(cb + t - c_begin), L.octave, (uint32_t)e};
                    ch[slot] = kp;
                    const ActEntry w = {kx, ky, resp, (slot << 8) | (uint32_t)e};
                    act_store(&act[ai], w);
                    const uint32_t ck = ai >> 6;
                    const bool fresh = !is_repeated && (ai & 63u) == 0u;
                    s_bmin[ck] = fresh ? ky : fminf(s_bmin[ck], ky);
                    s_bmax[ck] = fresh ? ky : fmaxf(s_bmax[ck], ky);
                }
                act_stores_done();
            }
        }
    }
    if (lane == 0) {
        ncache[frame] = overflowed ? max_kp + 1u : nslots;
        lvl_slot[(size_t)frame * (kMaxLevels + 1) + T.n] = nslots;
    }
}

// second pass (scale_space_extrema.rs:121-140): drop i if a LATER cache entry of class i+1 lies within
// size_i and has response >= response_i.  Thread per entry i.
// Where such an entry can sit: a slot pushed by a level-e candidate starts with class e and is only ever
// replaced by candidates of higher levels, so an entry of class c+1 lives in a slot pushed at level <= c+1, i.e.
// before lvl_slot[c+2] (the first-pass kernels record the first slot of every level).  Entry i therefore walks
// (i, lvl_slot[c+2]) only.  Slots are close to raster order, so the walk is pruned by the y range of every
// 64-slot chunk (exact: a chunk is skipped only when no entry of it can be within size_i).  k_chunk_yrange tabulates
// the ranges once per frame; a block copies the part its entries can need into LDS.  A wave then lists, 64 chunks at a
// time (lane <-> chunk), the chunks whose range meets the y window of its 64 entries, and visits them in order with the
// NEXT listed chunk's entries already requested (the walk is a chain of L2 round trips otherwise), broadcasting the
// entries lane by lane.  No barrier inside the walk.
__global__ __launch_bounds__(256) void k_chunk_yrange(const DevKp* __restrict__ cache, uint32_t max_kp,
                                                      const uint32_t* __restrict__ ncache, float2* __restrict__ yr,
                                                      uint32_t yr_stride)
{
    const int frame = blockIdx.y;
    const uint32_t n = min(ncache[frame], max_kp);
    const uint32_t ck = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (ck * 64u >= n) return;
    const uint32_t j = ck * 64u + lane;
    float ylo = 3.0e38f, yhi = -3.0e38f;
    if (j < n) ylo = yhi = cache[(size_t)frame * max_kp + j].y;
    for (int off = 32; off > 0; off >>= 1) {
        ylo = fminf(ylo, __shfl_xor(ylo, off));
        yhi = fmaxf(yhi, __shfl_xor(yhi, off));
    }
    if (lane == 0) yr[(size_t)frame * yr_stride + ck] = make_float2(ylo, yhi);
}

__global__ __launch_bounds__(256) void k_filter_upper(const DevKp* __restrict__ cache, uint32_t max_kp,
                                                      const uint32_t* __restrict__ ncache,
                                                      const uint32_t* __restrict__ lvl_slot, int nlev,
                                                      const float2* __restrict__ yr_tab, uint32_t yr_stride,
                                                      uint32_t* __restrict__ flag)
{
    __shared__ uint32_t s_P[kMaxLevels + 2];
    // {ymin, ymax} of chunk (cb0 + k): yr_stride entries of dynamic LDS — 1 KB at 8 192 keypoints a frame, not the 32 KB of the
    // largest context (which held the kernel to four blocks per CU: it waits on memory, and runs 185 -> ~100 us per 256 frames
    // with twice the waves)
    extern __shared__ __attribute__((aligned(8))) unsigned char s_dyn[];
    float2* s_yr = reinterpret_cast<float2*>(s_dyn);
    __shared__ uint32_t s_range[2];
    const int frame = blockIdx.y;
    const uint32_t n = min(ncache[frame], max_kp);
    const uint32_t i0 = blockIdx.x * 256;
    if (i0 >= n) return;
    const DevKp* ch = cache + (size_t)frame * max_kp;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if ((int)tid <= nlev) s_P[tid] = min(lvl_slot[(size_t)frame * (kMaxLevels + 1) + tid], n);
    if (tid == 0) {
        s_range[0] = 0xFFFFFFFFu;
        s_range[1] = 0u;
    }
    __syncthreads();
    const uint32_t i = i0 + tid;
    const bool valid = i < n;
    DevKp ki;
    ki.x = ki.y = ki.response = ki.size = 0.0f;
    ki.class_id = kMaxLevels;
    if (valid) ki = ch[i];
    const uint32_t want = ki.class_id + 1u;
    uint32_t jb = i + 1u, je = 0u;                            // [jb, je)
    if (valid && (int)want < nlev) je = s_P[min(want + 1u, (uint32_t)nlev)];
    const bool has = jb < je;
    uint32_t lo = has ? jb : 0xFFFFFFFFu, hi = has ? je : 0u;   // becomes the wave's union
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, (uint32_t)__shfl_xor((int)lo, off));
        hi = max(hi, (uint32_t)__shfl_xor((int)hi, off));
    }
    if (lane == 0 && lo < hi) {
        atomicMin(&s_range[0], lo);
        atomicMax(&s_range[1], hi);
    }
    jb = has ? jb : 0xFFFFFFFFu;
    je = has ? je : 0u;
    __syncthreads();
    const bool any_range = s_range[0] != 0xFFFFFFFFu;
    bool rep = false;
    if (any_range) {
        const uint32_t cb0 = s_range[0] >> 6, cb1 = (s_range[1] + 63u) >> 6;   // chunks [cb0, cb1)
        const float2* yt = yr_tab + (size_t)frame * yr_stride;
        for (uint32_t ck = cb0 + tid; ck < cb1; ck += 256) s_yr[ck - cb0] = yt[ck];
        __syncthreads();
        const float size2 = ki.size * ki.size;
        const float margin = ki.size * 1.001f + 0.01f;       // conservative: |dy| > margin  =>  dist > size^2
        // One walk per LEVEL REGION present in the wave (region e = the slots pushed at level e, in raster order).  A
        // wave's 64 entries are neighbours in cache order — a few rows — except where a region ends inside it: the last
        // rows of one and the first rows of the next together span the whole image, and a walk under their common window
        // would broadcast every entry of two classes to lanes that cannot use them (such a wave took as long as the rest
        // of its frame: 84 us of a single-frame call).  Taken region by region, each group's window is as narrow as any
        // other wave's.
        uint32_t reg = 0;
        for (int e = 1; e < nlev; ++e) reg += s_P[e] <= i ? 1u : 0u;
        unsigned long long todo = __ballot(has);
        while (todo) {
            const uint32_t cur = rl_u(reg, (uint32_t)__ffsll((long long)todo) - 1u);
            const bool act = has && reg == cur;
            todo &= ~__ballot(act);
            uint32_t glo = act ? jb : 0xFFFFFFFFu, ghi = act ? je : 0u;   // the group's union
            // its window in y (an entry outside it cannot be within `size` of any of the group's keypoints and is not
            // broadcast) and the classes it wants
            float wy_lo = act ? ki.y - margin : 3.0e38f, wy_hi = act ? ki.y + margin : -3.0e38f;
            uint32_t wmin = act ? want : 0xFFFFFFFFu, wmax = act ? want : 0u;
            for (int off = 32; off > 0; off >>= 1) {
                glo = min(glo, (uint32_t)__shfl_xor((int)glo, off));
                ghi = max(ghi, (uint32_t)__shfl_xor((int)ghi, off));
                wy_lo = fminf(wy_lo, __shfl_xor(wy_lo, off));
                wy_hi = fmaxf(wy_hi, __shfl_xor(wy_hi, off));
                wmin = min(wmin, (uint32_t)__shfl_xor((int)wmin, off));
                wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, off));
            }
            const uint32_t cend = (ghi + 63u) >> 6;
            for (uint32_t g0 = glo >> 6; g0 < cend; g0 += 64u) {
                // lane <-> chunk g0 + lane: listed when its y range meets the group's window
                const uint32_t mck = g0 + lane;
                bool listed = false;
                if (mck < cend) {
                    const float2 yr = s_yr[mck - cb0];
                    listed = wy_hi >= yr.x && wy_lo <= yr.y;
                }
                unsigned long long cm = __ballot(listed);
                if (!cm) continue;
                float ex = 0.f, ey = 0.f, er = 0.f, nx = 0.f, ny = 0.f, nr = 0.f;
                uint32_t ec = 0xFFFFFFFFu, nc = 0xFFFFFFFFu;
                uint32_t b = (uint32_t)__ffsll((long long)cm) - 1u;
                cm &= cm - 1ull;
                {
                    const uint32_t j = (g0 + b) * 64u + lane;
                    if (j < n) {
                        const DevKp kj = ch[j];
                        ex = kj.x; ey = kj.y; er = kj.response; ec = kj.class_id;
                    }
                }
                for (;;) {
                    const uint32_t ck = g0 + b;
                    const bool more = cm != 0ull;
                    if (more) {                               // the next listed chunk's entries: in flight behind this one's compares
                        b = (uint32_t)__ffsll((long long)cm) - 1u;
                        cm &= cm - 1ull;
                        const uint32_t j = (g0 + b) * 64u + lane;
                        nx = ny = nr = 0.f;
                        nc = 0xFFFFFFFFu;
                        if (j < n) {
                            const DevKp kj = ch[j];
                            nx = kj.x; ny = kj.y; nr = kj.response; nc = kj.class_id;
                        }
                    }
                    const float2 yr = s_yr[ck - cb0];
                    const uint32_t c_lo = ck * 64u, c_hi = c_lo + 64u;
                    const bool need = act && !rep && jb < c_hi && je > c_lo && ki.y + margin >= yr.x && ki.y - margin <= yr.y;
                    const unsigned long long nm0 = __ballot(need);
                    if (nm0) {
                        const bool cok = ec >= wmin && ec <= wmax && ey >= wy_lo && ey <= wy_hi;
                        unsigned long long m = __ballot(cok);
                        if (__popcll(m) <= __popcll(nm0)) {
                            // the chunk's candidates one by one to every lane (the common case: a dense group of 64 neighbours)
                            while (m) {
                                const uint32_t t = (uint32_t)__ffsll((long long)m) - 1u;
                                m &= m - 1ull;
                                const float qx = rl_f(ex, t), qy = rl_f(ey, t), qr = rl_f(er, t);
                                const uint32_t qc = rl_u(ec, t), jj = c_lo + t;
                                if (need && jj >= jb && jj < je && qc == want) {
                                    const float dx = ki.x - qx, dy = ki.y - qy;
                                    const float dist = dx * dx + dy * dy;
                                    if (dist <= size2 && ki.response <= qr) rep = true;
                                }
                            }
                        } else {
                            // the other way round — the few entries that need this chunk, one by one, against its 64 slots held by
                            // the lanes.  A group that is sparse in y (a level that pushed few slots of its own: two dozen entries
                            // over the whole image) lists every chunk of its range under its window, but each chunk is needed by
                            // one or two of its entries only; broadcasting the candidates cost such a wave 1 000 steps for 66.
                            unsigned long long nm = nm0, hitm = 0ull;
                            const uint32_t jj = c_lo + lane;
                            while (nm) {
                                const uint32_t t = (uint32_t)__ffsll((long long)nm) - 1u;
                                nm &= nm - 1ull;
                                const float bx = rl_f(ki.x, t), by = rl_f(ki.y, t), bs2 = rl_f(size2, t), br = rl_f(ki.response, t);
                                const uint32_t bw = rl_u(want, t), bjb = rl_u(jb, t), bje = rl_u(je, t);
                                const float dx = bx - ex, dy = by - ey;
                                const float dist = dx * dx + dy * dy;
                                const bool hit = cok && jj >= bjb && jj < bje && ec == bw && dist <= bs2 && br <= er;
                                if (__any(hit)) hitm |= 1ull << t;
                            }
                            if ((hitm >> lane) & 1ull) rep = true;
                        }
                    }
                    if (!more) break;
                    ex = nx; ey = ny; er = nr; ec = nc;
                }
            }
        }
    }
    if (valid) flag[(size_t)frame * max_kp + i] = rep ? 0u : 1u;
}

// ordered compaction of a per-frame keypoint list (and optionally its descriptors): block per frame.
template <bool WITH_DESC>
__global__ __launch_bounds__(1024) void k_compact(const DevKp* __restrict__ in, const akz_descriptor* __restrict__ din,
                                                  const uint32_t* __restrict__ flag, const uint32_t* __restrict__ n_in,
                                                  uint32_t in_stride, DevKp* __restrict__ out,
                                                  akz_descriptor* __restrict__ dout, uint32_t out_stride,
                                                  uint32_t* __restrict__ n_out, uint32_t* __restrict__ err,
                                                  const uint32_t* __restrict__ err_src, uint32_t* __restrict__ err_dst)
{
    __shared__ uint32_t s_wave[16];
    const int frame = blockIdx.x;
    // the host calls read the sticky overflow flag from the same (host-visible) block as the outputs: every kernel
    // that can raise it has completed before this one starts
    if (err_dst && blockIdx.x == 0 && threadIdx.x == 0) *err_dst = *err_src;
    const uint32_t n = min(n_in[frame], in_stride);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 1024) {
        uint32_t i = b0 + threadIdx.x;
        bool keep = i < n && flag[(size_t)frame * in_stride + i] != 0;
        unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t woff = 0, tot = 0;
        for (int q = 0; q < 16; ++q) {
            if (q < wv) woff += s_wave[q];
            tot += s_wave[q];
        }
        if (keep) {
            uint32_t o = base + woff + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            if (o < out_stride) {
                out[(size_t)frame * out_stride + o] = in[(size_t)frame * in_stride + i];
                if (WITH_DESC) {
                    const uint4* s = reinterpret_cast<const uint4*>(&din[(size_t)frame * in_stride + i]);
                    uint4* d = reinterpret_cast<uint4*>(&dout[(size_t)frame * out_stride + o]);
                    d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
                }
            }
        }
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        n_out[frame] = base;  // required count (may exceed out_stride -> AKZ_E_CAPACITY on the host side)
        if (base > out_stride && err) atomicOr(err, 4u);
    }
}

// ---------------------------------------------------------------------------------------------
// A13 + A14: sub-pixel refinement and main orientation, one wave per keypoint.
struct OriTables {
    signed char di[109], dj[109];  // sample offsets in the reference's (j outer, i inner) order
    float gw[109];                 // GAUSS25[id[j+6]][id[i+6]]
    float ang1[48];                // window starts: f32 accumulation of 0.15 (scale_space_extrema.rs:259-287)
    int n_win;
    // Which windows contain an angle depends only on where the angle falls among the windows' end points (plus 0
    // and 2 pi): bnd[] holds those values sorted (padded with +inf), m_open[r] the membership bits (bit = window)
    // of every angle strictly between bnd[r-1] and bnd[r], m_eq[r] those of the angle bnd[r] itself.  Built on
    // the host with ori_window_contains, the predicate the summation used to evaluate per (window, sample).
    float bnd[128];
    uint2 m_open[128], m_eq[128];
    // the same two tables interleaved for a lookup by scalar load: m_tab[2 r] = m_open[r], m_tab[2 r + 1] = m_eq[r], and
    // m_tab[256] = no window (the lanes of k_orient_describe that carry no sample)
    uint2 m_tab[257];
};

// scale_space_extrema.rs:261-287: is `ang` inside the window that starts at ang1 (width pi/3, wrapping at 2 pi)
__host__ __device__ __forceinline__ bool ori_window_contains(float ang1, float ang)
{
    const float PI_F = 3.14159274101257324219f;
    const float ang2 = (ang1 + PI_F / 3.0f > 2.0f * PI_F) ? ang1 - 5.0f * PI_F / 3.0f : ang1 + PI_F / 3.0f;
    const bool plain = ang1 < ang2, wrap = ang2 < ang1;
    return (plain && ang1 < ang && ang < ang2) ||
           (wrap && ((ang > 0.0f && ang < ang2) || (ang > ang1 && ang < 2.0f * PI_F)));
}

__device__ __forceinline__ float fast_atan2_equiv(float y, float x)
{
    // (y.atan2(x) + 2*PI).rem_euclid(2*PI) in f32 (scale_space_extrema.rs:242); the sum lies in
    // [pi, 3pi] so fmod is one exact conditional subtraction.
    const float two_pi = 2.0f * 3.14159274101257324219f;
    float a = akz_pm_atan2f(y, x) + two_pi;
    return a >= two_pi ? a - two_pi : a;
}

// ---------------------------------------------------------------------------------------------
// A12b in parallel.  The serial pass above costs ~6 ms per frame on one wave; it is exact but it is the whole
// latency of a single-frame call.  The same result can be computed without walking the candidates one by one:
//
//   * Everything a candidate c can ever match is static: an entry's position is K(n) = p_n * ratio_n + offset_n of
//     the candidate n that currently occupies it, its class is n's level, and c's test is
//     |F(c) - K(n)|^2 <= size_c^2 with class(n) in {level(c), level(c) - 1} (scale_space_extrema.rs:72-90).
//     k_sup_adj lists, for every c, the EARLIER candidates n that satisfy it (adj) and the reverse lists (radj).
//   * The pass is then a recurrence over records that depend on earlier candidates only:
//       slot(c)   = the cache slot c ends up writing (named by the candidate that pushed it), or none if dropped,
//       target(c) = the occupant c replaced, if any.
//     n still occupies its slot when c is processed iff slot(n) exists and no m < c in radj(n) has target(m) = n.
//     Among c's occupied neighbours the reference's linear scan finds the one in the lowest slot, i.e. the
//     smallest pusher index; c replaces it if its response is larger, is dropped otherwise, and pushes a new
//     slot when there is none.
//   * k_sup_resolve evaluates all records of a 1024-candidate chunk in parallel and repeats until a full sweep
//     changes nothing (the fixed point is unique by induction on the candidate order; chains inside a chunk are
//     short), chunk after chunk in candidate order.  The cache is the pushed slots in pusher order, each with the
//     data of its final occupant.
// Frames whose lists overflow the fixed capacities (kSupDeg neighbours, kSupCap candidates) are flagged and
// go through k_suppress instead, so the result is the same in every case.
constexpr int kSupDeg = kAkzSupDeg;    // neighbours kept per candidate (each direction)
constexpr uint32_t kSupNone = 0xFFFFFFFFu;

struct SupFrame {                      // per-frame views of the scratch arrays
    uint32_t* done;   // [kd] chunk k resolved: pushes up to and including it, + 1 (chunk-parallel mode)
    uint32_t* nradj;  // [cap]
    uint32_t* repl;   // [cap] a later candidate replaced this one in its slot
    uint2* state;     // [cap] {slot, target}
    uint32_t* nadj;   // [cap]
    float* resp;      // [cap]
    uint32_t* rank;   // [cap] exclusive count of pushes before the candidate
    uint32_t* adj;    // [cap][kSupDeg]
    uint32_t* radj;   // [cap][kSupDeg]
};

__device__ __forceinline__ SupFrame sup_frame(uint32_t* base, uint32_t cap, int frame, uint32_t nframes)
{
    // array-major layout over the frames of the call (akz_common.h: sup_scratch_words): done[n][kd], nradj[n][cap],
    // repl[n][cap] first (one memset clears them), then state(2), nadj, resp, rank, adj, radj
    const size_t kd = sup_done_words(cap);
    const size_t fc = (size_t)frame * cap, bc = (size_t)nframes * cap;
    uint32_t* p = base + (size_t)nframes * kd;
    SupFrame f;
    f.done = base + (size_t)frame * kd;
    f.nradj = p + fc;
    f.repl = p + bc + fc;
    f.state = reinterpret_cast<uint2*>(p + 2 * bc) + fc;
    f.nadj = p + 4 * bc + fc;
    f.resp = reinterpret_cast<float*>(p + 5 * bc) + fc;
    f.rank = p + 6 * bc + fc;
    f.adj = p + 7 * bc + fc * kSupDeg;
    f.radj = p + (7 + (size_t)kSupDeg) * bc + fc * kSupDeg;
    return f;
}

// level of global candidate index g and index inside the level, from the per-level prefix sums
__device__ __forceinline__ int sup_level(const uint32_t* base, int nlev, uint32_t g, uint32_t* i)
{
    int e = 0;
    while (e + 1 < nlev && g >= base[e + 1]) ++e;
    *i = g - base[e];
    return e;
}

// s_base[e] = candidates of the levels before e (s_base[nlev] = all of them), by the block's first wave: one load per
// level in parallel and a wave scan (a single thread walking the levels paid one L2 round trip per level — ~16 us at
// the head of every block).  Every thread of the block calls it; followed by a barrier.
__device__ __forceinline__ void sup_level_bases(uint32_t* s_base, const uint32_t* __restrict__ ncand_frame, int nlev,
                                                uint32_t max_cand)
{
    static_assert(kMaxLevels <= 64, "one wave scans the levels");
    if (threadIdx.x >= 64) return;
    const int lane = (int)threadIdx.x;
    const uint32_t v = lane < nlev ? min(ncand_frame[lane], max_cand) : 0u;
    uint32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane < nlev) s_base[lane] = inc - v;
    if (lane == nlev - 1) s_base[nlev] = inc;
    if (nlev == 0 && lane == 0) s_base[0] = 0u;
}

// Row-start table of a raster-sorted candidate list: rows[y] = the first candidate whose row is >= y, for y in [0, h]
// (rows[h] = the list's length).  k_sup_adj bounds its scans with two look-ups instead of a twelve-step bisection of
// the list (every step an L2 round trip).
__global__ __launch_bounds__(1024) void k_cand_rows(LevelTable T, const uint32_t* __restrict__ ncand,
                                                    const uint2* __restrict__ cand, uint32_t max_cand,
                                                    uint32_t* __restrict__ rows)
{
    const int level = blockIdx.x, frame = blockIdx.y;
    const uint32_t n = min(ncand[(size_t)frame * kAkzMaxLevels + level], max_cand);
    const uint32_t h = (uint32_t)T.L[level].h;
    const uint2* lst = cand + ((size_t)frame * kAkzMaxLevels + level) * max_cand;
    uint32_t* R = rows + (size_t)frame * T.rows_total + T.L[level].row_off;
    for (uint32_t j = threadIdx.x; j <= n; j += 1024) {
        const uint32_t r = j < n ? min(lst[j].x >> 16, h) : h;          // (the entry past the end takes the rows that are left)
        const uint32_t first = j > 0 ? (lst[j - 1].x >> 16) + 1u : 0u;  // rows not yet covered by an earlier candidate
        for (uint32_t y = first; y <= r; ++y) R[y] = j;
    }
}

__global__ __launch_bounds__(256) void k_sup_adj(LevelTable T, const uint32_t* __restrict__ ncand,
                                                 const uint2* __restrict__ cand, uint32_t max_cand, uint32_t* scratch,
                                                 uint32_t cap, uint32_t* __restrict__ fallback,
                                                 const uint32_t* __restrict__ rows)
{
    __shared__ uint32_t s_base[kMaxLevels + 1];
    const int frame = blockIdx.y;
    sup_level_bases(s_base, ncand + (size_t)frame * kAkzMaxLevels, T.n, max_cand);
    __syncthreads();
    const uint32_t N = s_base[T.n];
    if (N > cap && blockIdx.x == 0 && threadIdx.x == 0) fallback[frame] = 1u;
    if (N > cap) return;
    const SupFrame F = sup_frame(scratch, cap, frame, gridDim.y);
    const uint2* cd = cand + (size_t)frame * kAkzMaxLevels * max_cand;
    const uint32_t* RT = rows + (size_t)frame * T.rows_total;
    // (the grid is sized for a typical frame, not for `cap`: a block takes every gridDim.x-th group of 256 candidates)
    for (uint32_t g = blockIdx.x * 256 + threadIdx.x; g < N; g += gridDim.x * 256) {
    uint32_t i;
    const int e = sup_level(s_base, T.n, g, &i);
    const uint2 me = cd[(size_t)e * max_cand + i];
    const float ratio = ldexpf(1.0f, (int)T.L[e].octave);
    const float fx = (float)(me.x & 0xFFFFu) * ratio, fy = (float)(me.x >> 16) * ratio;
    const float size = T.L[e].kp_size, size2 = size * size;
    F.resp[g] = fabsf(__uint_as_float(me.y));
    F.state[g] = make_uint2(kSupNone, kSupNone);
    uint32_t cnt = 0;
    bool over = false;
    // the first kHits neighbours wait in registers: their reverse-list counters are then bumped by atomics that are all in
    // flight together (one round trip instead of one per neighbour: the hits were half of the kernel's time)
    constexpr uint32_t kHits = 6;
    uint32_t hits[kHits];
#pragma unroll
    for (uint32_t q = 0; q < kHits; ++q) hits[q] = 0u;
    for (int Lv = (e > 0 ? e - 1 : 0); Lv <= e; ++Lv) {
        const float rl = ldexpf(1.0f, (int)T.L[Lv].octave);
        const float hoff = 0.5f * (rl - 1.0f);
        const uint32_t nL = s_base[Lv + 1] - s_base[Lv];
        const uint2* lst = cd + (size_t)Lv * max_cand;
        const uint32_t lim = (Lv == e) ? i : nL;           // same level: earlier candidates only
        // rows of level Lv that can hold an entry within `size` of (fx, fy): conservative bounds
        const float lo = (fy - size - hoff) / rl - 1.0f, hi = (fy + size - hoff) / rl + 1.0f;
        const uint32_t ylo = lo > 0.0f ? (uint32_t)lo : 0u;
        const uint32_t yhi = hi > 0.0f ? (uint32_t)hi : 0u;
        // the candidates of rows [ylo, yhi] among the first `lim`: two look-ups in the row-start table
        const uint32_t hL = (uint32_t)T.L[Lv].h;
        const uint32_t* R = RT + T.L[Lv].row_off;
        const uint32_t a = min(R[min(ylo, hL)], lim), b = min(R[min(yhi + 1u, hL)], lim);
        auto test = [&](uint32_t xy, uint32_t j) {
            // the entry n = (Lv, j) would hold: K(n) = p * ratio + 0.5 (ratio - 1)   (:106-109)
            const float kx = (float)(xy & 0xFFFFu) * rl + hoff, ky = (float)(xy >> 16) * rl + hoff;
            const float dx = fx - kx, dy = fy - ky;
            if (dx * dx + dy * dy <= size2) {
                const uint32_t nidx = s_base[Lv] + j;
                if (cnt < kHits) {
#pragma unroll
                    for (uint32_t q = 0; q < kHits; ++q)
                        if (cnt == q) hits[q] = nidx;
                    ++cnt;
                    return;
                }
                if (cnt < (uint32_t)kSupDeg) F.adj[(size_t)g * kSupDeg + cnt] = nidx;
                else over = true;
                ++cnt;
                const uint32_t r = atomicAdd(&F.nradj[nidx], 1u);
                if (r < (uint32_t)kSupDeg) F.radj[(size_t)nidx * kSupDeg + r] = g;
                else over = true;
            }
        };
        // (the scan is a chain of memory round trips otherwise: eight entries are requested at a time, and the next eight
        // before the first of these is looked at)
        constexpr uint32_t kB = 8;
        uint32_t cur[kB], nxt[kB];
#pragma unroll
        for (uint32_t q = 0; q < kB; ++q) cur[q] = a + q < b ? lst[a + q].x : 0u;
        for (uint32_t j = a; j < b; j += kB) {
#pragma unroll
            for (uint32_t q = 0; q < kB; ++q) nxt[q] = j + kB + q < b ? lst[j + kB + q].x : 0u;
#pragma unroll
            for (uint32_t q = 0; q < kB; ++q)
                if (j + q < b) test(cur[q], j + q);
#pragma unroll
            for (uint32_t q = 0; q < kB; ++q) cur[q] = nxt[q];
        }
    }
    static_assert(kHits <= (uint32_t)kSupDeg, "the registers hold a prefix of the list");
    uint32_t rpos[kHits];
#pragma unroll
    for (uint32_t q = 0; q < kHits; ++q)
        if (q < cnt) F.adj[(size_t)g * kSupDeg + q] = hits[q];
#pragma unroll
    for (uint32_t q = 0; q < kHits; ++q) rpos[q] = q < cnt ? atomicAdd(&F.nradj[hits[q]], 1u) : 0u;
#pragma unroll
    for (uint32_t q = 0; q < kHits; ++q)
        if (q < cnt) {
            if (rpos[q] < (uint32_t)kSupDeg) F.radj[(size_t)hits[q] * kSupDeg + rpos[q]] = g;
            else over = true;
        }
    F.nadj[g] = min(cnt, (uint32_t)kSupDeg);
    if (over) fallback[frame] = 1u;
    }
}

// CHUNK_PARALLEL: one workgroup per (chunk, frame) — blockIdx.x = chunk — chained through the frame's done[] flags
// (a workgroup only ever waits for the chunk before it, which was dispatched before it); otherwise one workgroup per
// frame walks the chunks itself.  Few frames take the first form (the chunks' list fetches overlap and only the part
// that needs the earlier records is serial), a batch the second (every CU has a frame of its own).
template <bool CHUNK_PARALLEL>
__global__ __launch_bounds__(1024) void k_sup_resolve(LevelTable T, const uint32_t* __restrict__ ncand,
                                                      const uint2* __restrict__ cand, uint32_t max_cand,
                                                      uint32_t* scratch, uint32_t cap,
                                                      const uint32_t* __restrict__ fallback, DevKp* __restrict__ cache,
                                                      uint32_t max_kp, uint32_t* __restrict__ ncache,
                                                      uint32_t* __restrict__ err, uint32_t* __restrict__ lvl_slot)
{
    __shared__ uint32_t s_base[kMaxLevels + 1];
    __shared__ uint32_t s_scan[1024 / 64];
    __shared__ uint32_t s_run;
    const int frame = blockIdx.y;
    if (fallback[frame]) return;                 // k_suppress takes this frame
    const uint32_t tid = threadIdx.x;
    sup_level_bases(s_base, ncand + (size_t)frame * kAkzMaxLevels, T.n, max_cand);
    __syncthreads();
    const uint32_t N = s_base[T.n];
    const uint32_t nchunks = (N + 1023u) / 1024u;
    const uint32_t k0 = CHUNK_PARALLEL ? blockIdx.x : 0u;
    const uint32_t k1 = CHUNK_PARALLEL ? min(k0 + 1u, nchunks) : nchunks;
    if (N == 0) {
        if (k0 == 0) {
            if (tid == 0) ncache[frame] = 0u;
            if ((int)tid <= T.n) lvl_slot[(size_t)frame * (kMaxLevels + 1) + tid] = 0u;
        }
        return;
    }
    if (k0 >= nchunks) return;
    const SupFrame F = sup_frame(scratch, cap, frame, gridDim.y);
    // The records of a 1024-candidate chunk live in LDS while the chunk iterates.  Everything a candidate reads that
    // cannot change any more — its neighbour lists, the responses, and the records of candidates of EARLIER chunks,
    // which are final — is fetched once per chunk into registers (rounds of independent loads); a sweep of the
    // fixed-point iteration then touches LDS only.  Candidates with more than kSupRegN neighbours, kSupRegM reverse
    // entries per neighbour or kSupRegT in-chunk threats per neighbour (rare) evaluate from the lists in memory.
    constexpr int kSupRegN = 4, kSupRegM = 6, kSupRegT = 4;
    __shared__ uint2 s_state[1024];
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    uint32_t running = 0;
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t cb = k * 1024u;
        const uint32_t c = cb + tid;
        const bool on = c < N;
        s_state[tid] = make_uint2(kSupNone, kSupNone);
        uint32_t nn = 0;
        float rc = 0.0f;
        uint32_t nb[kSupRegN], nslot[kSupRegN], nth[kSupRegN], th[kSupRegN][kSupRegT], nr[kSupRegN], mm[kSupRegN][kSupRegM];
        float nresp[kSupRegN];
        bool rep_static[kSupRegN];
        bool generic = false;
#pragma unroll
        for (int a = 0; a < kSupRegN; ++a) {
            nb[a] = kSupNone; nslot[a] = kSupNone; nth[a] = 0u; nresp[a] = 0.0f; rep_static[a] = false; nr[a] = 0u;
#pragma unroll
            for (int q = 0; q < kSupRegT; ++q) th[a][q] = 0u;
#pragma unroll
            for (int q = 0; q < kSupRegM; ++q) mm[a][q] = kSupNone;
        }
        // ---- round A: the lists (nothing here depends on another chunk) ----
        if (on) {
            nn = F.nadj[c];
            rc = F.resp[c];
            generic = nn > (uint32_t)kSupRegN;
            if (!generic) {
#pragma unroll
                for (int a = 0; a < kSupRegN; ++a)
                    if ((uint32_t)a < nn) nb[a] = F.adj[(size_t)c * kSupDeg + a];
#pragma unroll
                for (int a = 0; a < kSupRegN; ++a)
                    if ((uint32_t)a < nn) {
                        nresp[a] = F.resp[nb[a]];
                        nr[a] = min(F.nradj[nb[a]], (uint32_t)kSupDeg);
                    }
#pragma unroll
                for (int a = 0; a < kSupRegN; ++a) {
                    if (nr[a] > (uint32_t)kSupRegM) generic = true;
#pragma unroll
                    for (int q = 0; q < kSupRegM; ++q)
                        if ((uint32_t)q < nr[a]) mm[a][q] = F.radj[(size_t)nb[a] * kSupDeg + q];
                }
            }
        }
        // ---- the chunk before this one is final (and with it every earlier one) ----
        if (CHUNK_PARALLEL && k > 0) {
            if (tid == 0) {
                uint32_t v;
                while ((v = __hip_atomic_load(&F.done[k - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u)
                    __builtin_amdgcn_s_sleep(2);
                s_run = v - 1u;
            }
            __syncthreads();
            running = s_run;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        // ---- round B: the final records of earlier chunks ----
        if (on && !generic) {
#pragma unroll
            for (int a = 0; a < kSupRegN; ++a)
                if ((uint32_t)a < nn && nb[a] < cb) nslot[a] = F.state[nb[a]].x;
#pragma unroll
            for (int a = 0; a < kSupRegN; ++a) {
#pragma unroll
                for (int q = 0; q < kSupRegM; ++q) {
                    const uint32_t m = mm[a][q];
                    if (m >= c) continue;                             // (kSupNone included) later candidates cannot have replaced n yet
                    if (m < cb) {
                        if (F.state[m].y == nb[a]) rep_static[a] = true;
                    } else if (nth[a] < (uint32_t)kSupRegT) {
#pragma unroll
                        for (int t = 0; t < kSupRegT; ++t)
                            if ((uint32_t)t == nth[a]) th[a][t] = m - cb;
                        ++nth[a];
                    } else {
                        generic = true;
                    }
                }
            }
        }
        __syncthreads();
        for (;;) {
            bool changed = false;
            if (on) {
                uint32_t best_slot = kSupNone, best_n = kSupNone;
                float best_resp = 0.0f;
                if (!generic) {
#pragma unroll
                    for (int a = 0; a < kSupRegN; ++a) {
                        if ((uint32_t)a >= nn) continue;
                        const uint32_t n = nb[a];
                        const uint32_t sl = n >= cb ? s_state[n - cb].x : nslot[a];
                        if (sl == kSupNone || sl >= best_slot) continue;   // dropped, or not the first in slot order
                        bool replaced = rep_static[a];
#pragma unroll
                        for (int t = 0; t < kSupRegT; ++t)
                            if ((uint32_t)t < nth[a] && s_state[th[a][t]].y == n) replaced = true;
                        if (!replaced) {
                            best_slot = sl;
                            best_n = n;
                            best_resp = nresp[a];
                        }
                    }
                } else {
                    for (uint32_t a = 0; a < nn; ++a) {
                        const uint32_t n = F.adj[(size_t)c * kSupDeg + a];
                        const uint32_t sl = n >= cb ? s_state[n - cb].x : F.state[n].x;
                        if (sl == kSupNone || sl >= best_slot) continue;
                        // still the occupant when c is processed?  not if an earlier-than-c candidate replaced it
                        bool replaced = false;
                        const uint32_t nrn = min(F.nradj[n], (uint32_t)kSupDeg);
                        for (uint32_t q = 0; q < nrn; ++q) {
                            const uint32_t m = F.radj[(size_t)n * kSupDeg + q];
                            if (m < c && (m >= cb ? s_state[m - cb].y : F.state[m].y) == n) {
                                replaced = true;
                                break;
                            }
                        }
                        if (!replaced) {
                            best_slot = sl;
                            best_n = n;
                            best_resp = F.resp[n];
                        }
                    }
                }
                uint2 st;
                if (best_n == kSupNone) st = make_uint2(c, kSupNone);                       // push
                else if (rc > best_resp) st = make_uint2(best_slot, best_n);                // is_repeated: in-place write
                else st = make_uint2(kSupNone, kSupNone);                                   // is_extremum = false
                const uint2 old = s_state[tid];
                if (old.x != st.x || old.y != st.y) {
                    s_state[tid] = st;
                    changed = true;
                }
            }
            if (!__syncthreads_or(changed ? 1 : 0)) break;
        }
        // ---- the chunk is final: records to memory, replaced occupants marked, pushes numbered ----
        const uint2 st = s_state[tid];
        if (on) {
            F.state[c] = st;
            if (st.y != kSupNone) F.repl[st.y] = 1u;
        }
        const bool push = on && st.x == c;
        const unsigned long long bal = __ballot(push);
        if (lane == 0) s_scan[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = running, tot = 0;
        for (uint32_t q = 0; q < 1024 / 64; ++q) {
            if (q < wv) off += s_scan[q];
            tot += s_scan[q];
        }
        if (on) F.rank[c] = off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        running += tot;
        if (CHUNK_PARALLEL) __threadfence();
        else __threadfence_block();
        __syncthreads();   // the next chunk reads these records from memory; s_state and s_scan are reused
        if (CHUNK_PARALLEL && tid == 0) __hip_atomic_store(&F.done[k], running + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (k1 < nchunks) return;                    // the workgroup of the last chunk finishes the frame
    if (tid == 0) {
        if (running > max_kp || running >= (1u << 24)) *err = 2u;
        ncache[frame] = running;     // unclipped (every reader takes min(., max_kp)): akz_last_overflow reports what was needed
    }
    // first slot pushed at every level (k_filter_upper bounds its walks with it): the pushes before the level's
    // first candidate
    if ((int)tid <= T.n) lvl_slot[(size_t)frame * (kMaxLevels + 1) + tid] = s_base[tid] < N ? F.rank[s_base[tid]] : running;
    // every slot's final occupant writes the entry
    const uint2* cd = cand + (size_t)frame * kAkzMaxLevels * max_cand;
    DevKp* ch = cache + (size_t)frame * max_kp;
    for (uint32_t c = tid; c < N; c += 1024) {
        const uint2 st = F.state[c];
        const uint32_t rp = F.repl[c];
        if (st.x == kSupNone || rp) continue;
        const uint32_t pos = F.rank[st.x];
        if (pos >= max_kp) continue;
        uint32_t i;
        const int e = sup_level(s_base, T.n, c, &i);
        const uint2 me = cd[(size_t)e * max_cand + i];
        const float ratio = ldexpf(1.0f, (int)T.L[e].octave);
        const float half_off = 0.5f * (ratio - 1.0f);
        const float fx = (float)(me.x & 0xFFFFu) * ratio, fy = (float)(me.x >> 16) * ratio;
        // keypoint.point = p * ratio + 0.5 * (ratio - 1)  (:106-109)
        // the angle field is not computed yet: it carries the candidate's index inside its level, which is where
        // the refinement finds the determinant values around the keypoint (k_refine overwrites it)
        DevKp kp = {fx + half_off, fy + half_off, fabsf(__uint_as_float(me.y)), T.L[e].kp_size, __uint_as_float(i),
                    T.L[e].octave, (uint32_t)e};
        ch[pos] = kp;
    }
}

// XCD-aware block order for the one-wave-per-keypoint kernels (workgroup b runs on XCD b % 8, observed):
// consecutive keypoints are spatial neighbours, so each XCD gets a contiguous run of (frame, keypoint block)
// ids and its L2 keeps the pyramid lines the neighbours share.  Bijective for any grid size.
__device__ __forceinline__ uint2 xcd_block2(uint32_t bx, uint32_t by, uint32_t gx, uint32_t gy)
{
    const uint32_t nwg = gx * gy, orig = bx + gx * by;
    const uint32_t xcd = orig & 7u, q = nwg >> 3, r = nwg & 7u;
    const uint32_t t = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (orig >> 3);
    const uint32_t y = t / gx;
    return make_uint2(t - y * gx, y);
}

// do_subpixel_refinement, scale_space_extrema.rs:301-347.  Moves the keypoint to the vertex of the quadratic through the nine
// determinant values around it and doubles its size; false (the keypoint untouched but for the angle) when the vertex lies
// more than a pixel away.
// Ldet around (x, y): the keypoint sits on the pixel of the candidate that occupies its cache slot, and the candidate list
// carries those nine values (k_deriv_second_cand*, k_cand_sort), so the Ldet planes are never read here.  kp->angle holds
// the candidate's index inside its level (k_sup_resolve / k_suppress) until it is overwritten below.
__device__ __forceinline__ bool subpixel_fit(const LevelTable& T, const float* __restrict__ cand_nb, uint32_t max_cand, int frame,
                                             DevKp* kp)
{
    const LevelDesc* Lp = &T.L[kp->class_id];
    const float ratio = ldexpf(1.0f, (int)kp->octave);
    int x = (int)sat_u32(roundf(kp->x / ratio));
    int y = (int)sat_u32(roundf(kp->y / ratio));
    const uint32_t cidx = __float_as_uint(kp->angle);
    const float4* nbp = reinterpret_cast<const float4*>(cand_nb + (((size_t)frame * kAkzMaxLevels + kp->class_id) * max_cand + cidx) * 8);
    const float4 n0 = nbp[0], n1 = nbp[1];
    kp->angle = 0.0f;
    float x_i = kp->response;   // Ldet at the pixel (> threshold > 0, so |v| = v)
    float x_m_y_m = n0.x, y_m = n0.y, x_p_y_m = n0.z, x_m = n0.w, x_p = n1.x, x_m_y_p = n1.y, y_p = n1.z, x_p_y_p = n1.w;
    float d_x = 0.5f * (x_p - x_m);
    float d_y = 0.5f * (y_p - y_m);
    float d_xx = x_p + x_m - 2.0f * x_i;
    float d_yy = y_p + y_m - 2.0f * x_i;
    float d_xy = 0.25f * (x_p_y_p + x_m_y_m) - 0.25f * (x_p_y_m + x_m_y_p);
    float inv_det_a = 1.0f / (d_xx * d_yy - d_xy * d_xy);
    float inv_a0 = inv_det_a * d_yy;
    float inv_a1 = inv_det_a * -d_xy;
    float inv_a2 = inv_det_a * -d_xy;
    float inv_a3 = inv_det_a * d_xx;
    float dst0 = -d_x * inv_a0 + -d_y * inv_a1;
    float dst1 = -d_x * inv_a2 + -d_y * inv_a3;
    const bool keep = fabsf(dst0) <= 1.0f && fabsf(dst1) <= 1.0f;
    if (keep) {
        float nx = (float)x + dst0, ny = (float)y + dst1;
        float power = ldexpf(1.0f, (int)Lp->octave);
        kp->x = nx * power + 0.5f * (power - 1.0f);
        kp->y = ny * power + 0.5f * (power - 1.0f);
        kp->size = kp->size * 2.0f;
    }
    return keep;
}

__global__ __launch_bounds__(256) void k_refine(LevelTable T, const OriTables* __restrict__ ori_p,
                                                const DevKp* __restrict__ in,
                                                const uint32_t* __restrict__ n_in, uint32_t stride,
                                                DevKp* __restrict__ out, uint32_t* __restrict__ flag,
                                                uint32_t* __restrict__ err, const float* __restrict__ cand_nb,
                                                uint32_t max_cand)
{
    __shared__ float2 s_r[4][112];           // weighted {Lx, Ly} of every sample
    __shared__ uint32_t s_msk[4][112][2];   // per sample: the windows that contain its angle (bit = window)
    __shared__ float s_bnd[128];
    __shared__ uint2 s_mopen[128], s_meq[128];
    const OriTables& c_ori = *ori_p;
    if (threadIdx.x < 128) {
        s_bnd[threadIdx.x] = c_ori.bnd[threadIdx.x];
        s_mopen[threadIdx.x] = c_ori.m_open[threadIdx.x];
        s_meq[threadIdx.x] = c_ori.m_eq[threadIdx.x];
    }
    __syncthreads();
    const uint2 blk = xcd_block2(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
    const int frame = (int)blk.y;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t n = min(n_in[frame], stride);
    const uint32_t ki = blk.x * 4 + wv;
    const bool active = ki < n;  // wave-uniform; inactive waves still join the block barriers
    DevKp kp;
    bool keep = false;
    const LevelDesc* Lp = &T.L[0];
    if (active) {
        kp = in[(size_t)frame * stride + ki];
        Lp = &T.L[kp.class_id];
        keep = subpixel_fit(T, cand_nb, max_cand, frame, &kp);   // every lane computes the same scalars
    }
    // compute_main_orientation, :229-288
    if (active && keep) {
        const float oratio = (float)(1u << Lp->octave);
        const float s = roundf(0.5f * kp.size / oratio);
        const float xf = kp.x / oratio, yf = kp.y / oratio;
        const float2* LXY = Lp->Lxy + (size_t)frame * Lp->fs;
        for (int idx = lane; idx < 109; idx += 64) {
            unsigned iy = sat_u32(roundf(yf + (float)c_ori.dj[idx] * s));
            unsigned ix = sat_u32(roundf(xf + (float)c_ori.di[idx] * s));
            if (ix >= (unsigned)Lp->w || iy >= (unsigned)Lp->h) {  // the reference would panic here
                atomicOr(err, 8u);
                ix = min(ix, (unsigned)Lp->w - 1u);
                iy = min(iy, (unsigned)Lp->h - 1u);
            }
            float g = c_ori.gw[idx];
            float2 dxy = LXY[(size_t)iy * Lp->w + ix];
            float rx = g * dxy.x;
            float ry = g * dxy.y;
            s_r[wv][idx] = make_float2(rx, ry);
            // Window membership of this sample (:261-287) from the end-point table: the summation below (windows
            // across the lanes, samples in order) then needs one bit test per sample instead of the predicate.
            const float ang = fast_atan2_equiv(ry, rx);
            // r = number of end points below ang (branch-free binary search over the padded table)
            int r = 0;
#pragma unroll
            for (int step = 64; step > 0; step >>= 1) r += s_bnd[r + step - 1] < ang ? step : 0;
            const uint2 mm = (r < 128 && s_bnd[r & 127] == ang) ? s_meq[r & 127] : s_mopen[r & 127];
            const uint32_t mlo = mm.x, mhi = mm.y;
            s_msk[wv][idx][0] = mlo;
            s_msk[wv][idx][1] = mhi;
        }
    }
    __syncthreads();
    if (active && keep) {
        float val = -1.0f, sum_x = 0.0f, sum_y = 0.0f;
        if (lane < c_ori.n_win) {
            // branch-free: a sample outside the window adds +0.0, which leaves the sums bit-identical to skipping
            // it (they start at +0 and x + (+0) = x for every x but -0, which a sum that started at +0 never is)
            const int word = lane >> 5, bit = lane & 31;
            typedef float v2f __attribute__((ext_vector_type(2)));
            v2f sum = {0.0f, 0.0f};                       // {sum_x, sum_y}: one packed add per sample
#pragma unroll 4
            for (int k = 0; k < 109; ++k) {
                const bool in = (s_msk[wv][k][word] >> bit) & 1u;
                const float2 r = s_r[wv][k];
                sum += (v2f){in ? r.x : 0.0f, in ? r.y : 0.0f};
            }
            sum_x = sum.x;
            sum_y = sum.y;
            val = sum_x * sum_x + sum_y * sum_y;
        }
        // the serial loop keeps the FIRST window whose val exceeds every earlier one: the earliest
        // window holding the overall maximum, provided that maximum is > 0.
        float m = val;
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        unsigned long long bal = __ballot(val == m && lane < c_ori.n_win);
        int win = __ffsll((long long)bal) - 1;
        float best_sx = __shfl(sum_x, win), best_sy = __shfl(sum_y, win);
        kp.angle = (m > 0.0f) ? fast_atan2_equiv(best_sy, best_sx) : 0.0f;
    }
    if (active && lane == 0) {
        out[(size_t)frame * stride + ki] = kp;
        flag[(size_t)frame * stride + ki] = keep ? 1u : 0u;
    }
}

// ---------------------------------------------------------------------------------------------
// A15: sort by response descending (ties: lower pre-sort index first), truncate to maximum_features — and the
// visiting order of the descriptor stage — as RANK sorts: the keys are unique (the index rides in the low bits),
// so the sorted position of an element is the number of keys smaller than its own.  Every keypoint counts that
// against all keys of its frame (tiles of 1024 keys through LDS, every lane reading the same address: a
// broadcast), 256 keypoints per block: n^2 comparisons spread over the whole chip instead of one block's bitonic
// network (a single 1080p frame: 154 -> ~20 us per sort; no 128 KB LDS buffer, no capacity limit).
//   RANK_RESPONSE: key = (~response_bits, index); out[rank] = keypoint for rank < maximum_features
//   RANK_SPATIAL:  key = (level, 32-px tile row, tile column, index); perm[rank] = index.  The response-sorted list
//                  is spatially random, so consecutive keypoints (one per wave of the descriptor kernel) would
//                  sample unrelated patches; the kernel walks this permutation and still writes each descriptor
//                  to its keypoint's own slot, so the output order (response descending) is untouched.
enum { RANK_RESPONSE = 0, RANK_SPATIAL = 1 };

template <int MODE>
__device__ __forceinline__ unsigned long long rank_key(const DevKp& kp, uint32_t i, int tile_shift)
{
    if (MODE == RANK_RESPONSE) {
        // responses are |Ldet| > 0: the IEEE bit pattern is monotone in the value
        return ((unsigned long long)(~__float_as_uint(kp.response)) << 32) | (unsigned long long)i;
    }
    const float ratio = (float)(1u << kp.octave);
    const uint32_t tx = (uint32_t)max(kp.x / ratio, 0.0f) >> tile_shift, ty = (uint32_t)max(kp.y / ratio, 0.0f) >> tile_shift;
    const uint32_t sk = (min(kp.class_id, 63u) << 24) | (min(ty, 4095u) << 12) | min(tx, 4095u);
    return ((unsigned long long)sk << 32) | (unsigned long long)i;
}

constexpr int kRankI = 32, kRankJ = 8;   // keypoints per block x slices of a key tile (kRankI * kRankJ = 256 threads)
template <int MODE>
__global__ __launch_bounds__(256) void k_rank_sort(const DevKp* __restrict__ in, const uint32_t* __restrict__ n_in,
                                                   uint32_t stride, uint32_t max_features, int tile_shift,
                                                   DevKp* __restrict__ out, uint32_t* __restrict__ n_out,
                                                   uint32_t* __restrict__ perm)
{
    // a block ranks kRankI keypoints; its 256 threads split every 1024-key tile kRankJ ways, so a thread compares
    // against n / kRankJ keys and the chip holds n / kRankI blocks per frame (single frame of 4 600 keypoints:
    // 145 blocks x 577 compares per thread instead of 19 x 4 616)
    __shared__ unsigned long long s_key[1024];
    __shared__ uint32_t s_part[kRankJ][kRankI];
    const int frame = blockIdx.y;
    const uint32_t n = min(n_in[frame], stride);
    if (blockIdx.x * (uint32_t)kRankI >= n && !(blockIdx.x == 0 && MODE == RANK_RESPONSE)) return;    // whole block
    const DevKp* src = in + (size_t)frame * stride;
    const uint32_t ii = threadIdx.x & (kRankI - 1), js = threadIdx.x / kRankI;
    const uint32_t i = blockIdx.x * (uint32_t)kRankI + ii;
    DevKp me;
    unsigned long long mine = ~0ull;
    if (i < n) {
        me = src[i];
        mine = rank_key<MODE>(me, i, tile_shift);
    }
    uint32_t rank = 0;
    constexpr uint32_t kSlice = 1024 / kRankJ;
    for (uint32_t t0 = 0; t0 < n; t0 += 1024) {
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < 1024; j += 256)
            s_key[j] = t0 + j < n ? rank_key<MODE>(src[t0 + j], t0 + j, tile_shift) : ~0ull;
        __syncthreads();
        const uint32_t m = min(1024u, n - t0);
        const uint32_t j0 = js * kSlice, j1 = min(m, j0 + kSlice);
#pragma unroll 8
        for (uint32_t j = j0; j < j1; ++j) rank += s_key[j] < mine ? 1u : 0u;
    }
    s_part[js][ii] = rank;
    __syncthreads();
    if (js == 0 && i < n) {
        rank = 0;
#pragma unroll
        for (int k = 0; k < kRankJ; ++k) rank += s_part[k][ii];
        if (MODE == RANK_RESPONSE) {
            if (rank < max_features) out[(size_t)frame * stride + rank] = me;
            if (perm) perm[(size_t)frame * stride + i] = rank;    // pre-sort order as the descriptor stage's visiting order
        } else {
            perm[(size_t)frame * stride + rank] = i;
        }
    }
    if (MODE == RANK_RESPONSE && blockIdx.x == 0 && threadIdx.x == 0) n_out[frame] = n < max_features ? n : max_features;
}

// The same two orders by one block per frame: bitonic networks of 64-bit keys in LDS (lists beyond 16384 keys through
// the frame's global key scratch, akz_common.h).  A batch of many frames keeps every CU busy with one block per
// frame, and there the networks cost less than the n^2 comparisons (74 vs 190 us per 64 frames of ~5 000 keypoints):
// akz_run_keypoints picks by batch size.
__global__ __launch_bounds__(1024) void k_sort(const DevKp* __restrict__ in, const uint32_t* __restrict__ n_in,
                                               uint32_t stride, uint32_t max_features, DevKp* __restrict__ out,
                                               uint32_t* __restrict__ n_out, unsigned long long* __restrict__ gkeys,
                                               uint32_t gstride, uint32_t lds_keys, uint32_t* __restrict__ perm_raster)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem);
    const int frame = blockIdx.x;
    const uint32_t n = min(n_in[frame], stride);
    uint32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    const DevKp* src = in + (size_t)frame * stride;
    // lists longer than the LDS buffer sort through the frame's global key scratch (akz_common.h)
    if (n <= kRadixSortMax) {
        // Up to kRadixSortMax keypoints: a stable LSD radix sort of the 32-bit keys in LDS (akz_common.h) instead of the
        // bitonic network over padded 64-bit keys (159 -> 38 us per 64 frames of ~5 000 keypoints).  Stability does the
        // tie-break: equal responses keep their pre-sort order, which is the (response desc, index asc) order.
        uint32_t* rk = reinterpret_cast<uint32_t*>(smem);     // [kRadixSortMax] keys by element
        uint32_t* ia = rk + kRadixSortMax;                    // [kRadixSortMax] element ids, ping
        uint32_t* ib = ia + kRadixSortMax;                    // [kRadixSortMax] pong
        uint32_t* wh = ib + kRadixSortMax;                    // [16][256] per-wave digit counts / running offsets
        __shared__ uint32_t s_tot[256];
        const uint32_t tid = threadIdx.x;
        for (uint32_t i = tid; i < n; i += 1024) {
            rk[i] = ~__float_as_uint(src[i].response);        // responses are |Ldet| > 0: the bit pattern is monotone
            ia[i] = i;
        }
        const uint32_t* sorted = lds_radix_sort_ids(rk, ia, ib, wh, s_tot, n, 4);   // (its first barrier orders the fill)
        const uint32_t m = n < max_features ? n : max_features;
        for (uint32_t i = tid; i < m; i += 1024) {
            const uint32_t from = sorted[i];
            out[(size_t)frame * stride + i] = src[from];
            if (perm_raster) perm_raster[(size_t)frame * stride + from] = i;
        }
        if (tid == 0) n_out[frame] = m;
        return;
    }
    const bool big = np2 > lds_keys;
    unsigned long long* key = big ? gkeys + (size_t)frame * gstride : lds;
    for (uint32_t i = threadIdx.x; i < np2; i += 1024) {
        unsigned long long k = ~0ull;
        if (i < n) {
            // responses are |Ldet| > 0: the IEEE bit pattern is monotone in the value
            uint32_t rb = __float_as_uint(src[i].response);
            k = ((unsigned long long)(~rb) << 32) | (unsigned long long)i;
        }
        key[i] = k;
    }
    __threadfence_block();
    __syncthreads();
    if (big) bitonic_sort_big_u64<1024>(key, np2, lds, lds_keys);
    else bitonic_sort_lds_u64<1024>(key, np2);
    uint32_t m = n < max_features ? n : max_features;
    for (uint32_t i = threadIdx.x; i < m; i += 1024) {
        const uint32_t from = (uint32_t)(key[i] & 0xFFFFFFFFull);
        out[(size_t)frame * stride + i] = src[from];
        // visiting order of the descriptor stage = the pre-sort order (level-major, close to raster): see akz_run_keypoints
        if (perm_raster) perm_raster[(size_t)frame * stride + from] = i;
    }
    if (threadIdx.x == 0) n_out[frame] = m;
}

// Visiting order for the descriptor stage.  The response-sorted list is spatially random, so four
// consecutive keypoints (one workgroup) sample four unrelated 40-80 px patches and thrash the 32 KB L1.
// This kernel sorts the keypoint INDICES by (level, 32-px tile row, 32-px tile column); k_describe_fast
// walks that permutation and still writes each descriptor to its keypoint's own slot, so the output order
// (response descending) is untouched.
__global__ __launch_bounds__(1024) void k_spatial_order(LevelTable T, const DevKp* __restrict__ in,
                                                        const uint32_t* __restrict__ n_in, uint32_t stride,
                                                        uint32_t* __restrict__ perm, int tile_shift,
                                                        unsigned long long* __restrict__ gkeys, uint32_t gstride, uint32_t lds_keys)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* lds = reinterpret_cast<unsigned long long*>(smem);
    const int frame = blockIdx.x;
    const uint32_t n = min(n_in[frame], stride);
    uint32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    const DevKp* src = in + (size_t)frame * stride;
    const bool big = np2 > lds_keys;
    unsigned long long* key = big ? gkeys + (size_t)frame * gstride : lds;
    for (uint32_t i = threadIdx.x; i < np2; i += 1024) {
        unsigned long long k = ~0ull;
        if (i < n) {
            const DevKp kp = src[i];
            const float ratio = (float)(1u << kp.octave);
            uint32_t tx = (uint32_t)max(kp.x / ratio, 0.0f) >> tile_shift, ty = (uint32_t)max(kp.y / ratio, 0.0f) >> tile_shift;
            uint32_t sk = (min(kp.class_id, 63u) << 24) | (min(ty, 4095u) << 12) | min(tx, 4095u);
            k = ((unsigned long long)sk << 32) | (unsigned long long)i;
        }
        key[i] = k;
    }
    __threadfence_block();
    __syncthreads();
    if (big) bitonic_sort_big_u64<1024>(key, np2, lds, lds_keys);
    else bitonic_sort_lds_u64<1024>(key, np2);
    for (uint32_t i = threadIdx.x; i < n; i += 1024) perm[(size_t)frame * stride + i] = (uint32_t)(key[i] & 0xFFFFFFFFull);
}

// The same (level, tile) grouping as a COUNTING sort: the tiles of all levels are a few thousand buckets (10 900 at
// 1080p), so a block counts its frame's keypoints per bucket in LDS, scans the counts and scatters the indices — three
// passes over the list instead of a bitonic network over padded 64-bit keys (153 -> ~20 us per 64 frames).  Inside a
// tile the order is whatever the atomics produce: the permutation only decides in which order the descriptor kernel
// visits keypoints, never what it writes where.  The host falls back to k_spatial_order when the bucket count does
// not fit (kTileOrderMaxBuckets).
constexpr uint32_t kTileOrderMaxBuckets = 15 * 1024;
__global__ __launch_bounds__(1024) void k_tile_order(LevelTable T, const DevKp* __restrict__ in,
                                                     const uint32_t* __restrict__ n_in, uint32_t stride,
                                                     uint32_t* __restrict__ perm, int tile_shift)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem);            // [nb]
    __shared__ uint32_t s_lbase[kMaxLevels + 1], s_ntx[kMaxLevels], s_nty[kMaxLevels];
    __shared__ uint32_t s_wave[16];
    const int frame = blockIdx.x;
    const uint32_t n = min(n_in[frame], stride);
    const DevKp* src = in + (size_t)frame * stride;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid == 0) {
        uint32_t base = 0;
        for (int e = 0; e < T.n; ++e) {
            const uint32_t ntx = ((uint32_t)(T.L[e].w - 1) >> tile_shift) + 1u, nty = ((uint32_t)(T.L[e].h - 1) >> tile_shift) + 1u;
            s_lbase[e] = base;
            s_ntx[e] = ntx;
            s_nty[e] = nty;
            base += ntx * nty;
        }
        s_lbase[T.n] = base;
    }
    __syncthreads();
    const uint32_t nb = s_lbase[T.n];
    for (uint32_t b = tid; b < nb; b += 1024) hist[b] = 0u;
    __syncthreads();
    auto bucket = [&](const DevKp& kp) {
        const uint32_t e = min(kp.class_id, (uint32_t)T.n - 1u);
        const float ratio = (float)(1u << kp.octave);
        const uint32_t tx = min((uint32_t)max(kp.x / ratio, 0.0f) >> tile_shift, s_ntx[e] - 1u);
        const uint32_t ty = min((uint32_t)max(kp.y / ratio, 0.0f) >> tile_shift, s_nty[e] - 1u);
        return s_lbase[e] + ty * s_ntx[e] + tx;
    };
    for (uint32_t i = tid; i < n; i += 1024) atomicAdd(&hist[bucket(src[i])], 1u);
    __syncthreads();
    // exclusive scan of the counts: a contiguous run of buckets per thread, then the runs across the block
    const uint32_t per = (nb + 1023u) / 1024u, b0 = tid * per, b1 = min(nb, b0 + per);
    uint32_t run = 0;
    for (uint32_t b = b0; b < b1; ++b) run += hist[b];
    uint32_t incl = run;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
        if ((int)lane >= off) incl += v;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    uint32_t before = incl - run;
    for (uint32_t q = 0; q < wv; ++q) before += s_wave[q];
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t cnt = hist[b];
        hist[b] = before;
        before += cnt;
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += 1024) {
        const uint32_t pos = atomicAdd(&hist[bucket(src[i])], 1u);
        perm[(size_t)frame * stride + pos] = i;
    }
}

// ---------------------------------------------------------------------------------------------
// A16 + A17: M-LDB descriptor, one wave per keypoint.  Lane c (< n_cells) accumulates cell c of the
// three sampling grids sequentially in the reference's (k outer, l inner) order; the comparisons
// are then spread over the lanes one output byte each.
struct DescTables {
    // per cell: grid-local origin (i, j) and sample step of its grid; value slot base
    signed char ci[32], cj[32];
    unsigned char step[32];
    unsigned char vbase[32];        // index of the cell's first value in the per-keypoint value array
    int n_cells;                    // 4 + 9 + 16 = 29
    int nch;                        // descriptor_channels
    int n_bits;                     // nch * (6 + 36 + 120)
    unsigned char cmp_a[512], cmp_b[512];  // value indices compared for bit b: bit = v[a] > v[b]
};

__global__ __launch_bounds__(256) void k_describe(LevelTable T, const DescTables* __restrict__ desc_p,
                                                  const DevKp* __restrict__ in,
                                                  const uint32_t* __restrict__ n_in, uint32_t stride,
                                                  akz_descriptor* __restrict__ out, uint32_t* __restrict__ flag)
{
    __shared__ float s_val[4][96];
    const DescTables& c_desc = *desc_p;
    const int frame = blockIdx.y;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t n = min(n_in[frame], stride);
    const uint32_t ki = blockIdx.x * 4 + wv;
    const bool active = ki < n;
    bool oob = false;
    if (active) {
        const DevKp kp = in[(size_t)frame * stride + ki];
        const LevelDesc& L = T.L[kp.class_id];
        // get_mldb_descriptor, descriptors.rs:66-72
        const float ratio = (float)(1u << kp.octave);
        const float scale = roundf(0.5f * kp.size / ratio);
        const float xf = kp.x / ratio, yf = kp.y / ratio;
        const float co = akz_pm_cosf(kp.angle), si = akz_pm_sinf(kp.angle);
        if (lane < c_desc.n_cells) {
            const float* LT = L.Lt + (size_t)frame * L.fs;
            const float2* LXY = L.Lxy + (size_t)frame * L.fs;
            const int i0 = c_desc.ci[lane], j0 = c_desc.cj[lane], st = c_desc.step[lane];
            const int nch = c_desc.nch;
            float di = 0.0f, dx = 0.0f, dy = 0.0f;
            uint32_t nsamples = 0;
            // mldb_fill_values, descriptors.rs:123-159
            for (int k = i0; k < i0 + st && !oob; ++k) {
                for (int l = j0; l < j0 + st; ++l) {
                    float lf = (float)l, kf = (float)k;
                    float sample_y = yf + (lf * co * scale + kf * si * scale);
                    float sample_x = xf + (-lf * si * scale + kf * co * scale);
                    int y1 = sat_i32(roundf(sample_y));
                    int x1 = sat_i32(roundf(sample_x));
                    if (x1 < 0 || x1 >= L.w || y1 < 0 || y1 >= L.h) {
                        oob = true;  // Error::SampleOutOfBounds -> the keypoint is dropped (descriptors.rs:28)
                        break;
                    }
                    size_t p = (size_t)y1 * L.w + x1;
                    float ri = LT[p];
                    di += ri;
                    if (nch > 1) {
                        float2 dxy = LXY[p];
                        float rx = dxy.x, ry = dxy.y;
                        if (nch == 2) {
                            dx += sqrtf(rx * rx + ry * ry);
                        } else {
                            float rry = rx * co + ry * si;
                            float rrx = -rx * si + ry * co;
                            dx += rrx;
                            dy += rry;
                        }
                    }
                    nsamples += 1;
                }
            }
            if (!oob) {
                float ns = (float)nsamples;
                di /= ns;
                dx /= ns;
                dy /= ns;
                int vb = c_desc.vbase[lane];
                s_val[wv][vb] = di;
                if (nch > 1) s_val[wv][vb + 1] = dx;
                if (nch > 2) s_val[wv][vb + 2] = dy;
            }
        }
        oob = __any(oob);
    }
    __syncthreads();
    if (active) {
        // mldb_binary_comparisons, descriptors.rs:181-202: bit b -> byte b>>3, position b&7 (LSB first)
        uint32_t byte = 0;
        if (!oob) {
            for (int t = 0; t < 8; ++t) {
                int b = lane * 8 + t;
                if (b < c_desc.n_bits) {
                    float va = s_val[wv][c_desc.cmp_a[b]], vb = s_val[wv][c_desc.cmp_b[b]];
                    byte |= (va > vb ? 1u : 0u) << t;
                }
            }
        }
        out[(size_t)frame * stride + ki].bytes[lane] = (uint8_t)byte;
        if (lane == 0) flag[(size_t)frame * stride + ki] = oob ? 0u : 1u;
    }
}

// ---------------------------------------------------------------------------------------------
// Fast path of A16 + A17 for the reference's default pattern (descriptor_pattern_size 10, 3 channels:
// grids of 2x2 / 3x3 / 4x4 cells with sample steps 10 / 7 / 5).  One wave per keypoint:
//   gather   lane <-> lattice sample, consecutive lanes = consecutive samples of a lattice row, i.e.
//            neighbouring pixels: the wave's loads fall on a few cache lines instead of 64, and {Lx,Ly} is one
//            8-byte load.  Each sample's (Lt, rotated dx, rotated dy) goes to the wave's LDS segment.
//   reduce   lane <-> cell: the cell's samples are summed from LDS sequentially in the reference's
//            (k outer, l inner) order (descriptors.rs:123-159) — the order is what makes the f32 sums
//            bit-exact, so there is no tree reduction.
// A wave's DS instructions execute in order, so the reduce phase sees the gather phase's writes without
// a barrier; waves never share LDS here.
// Cell means of one M-LDB grid (step ST, SIDE x SIDE cells) from the wave's lattice values: lane <-> (cell,
// channel), every sum sequential in mldb_fill_values' order (descriptors.rs:123-159), then / nsamples.
template <int ST, int SIDE, int VBASE>
__device__ __forceinline__ void desc_cells(const float* s_ri, const float* s_dx, const float* s_dy, float* s_val, int lane)
{
    constexpr int LAT = 21;
    if (lane >= SIDE * SIDE * 3) return;
    const int cell = lane / 3, ch = lane - cell * 3;
    const int ci = cell / SIDE, cj = cell - ci * SIDE;          // i outer (k), j inner (l): descriptors.rs:117-118
    const float* src = (ch == 0 ? s_ri : (ch == 1 ? s_dx : s_dy)) + (ci * ST) * LAT + cj * ST;
    float acc = 0.0f;
#pragma unroll
    for (int kk = 0; kk < ST; ++kk)
#pragma unroll
        for (int ll = 0; ll < ST; ++ll) acc += src[kk * LAT + ll];
    s_val[VBASE + cell * 3 + ch] = acc / (float)(ST * ST);
}

// The same, returning the mean instead of storing it (k_orient_describe keeps the three grids' means in registers until
// the lattice planes are dead and stores them over the planes).
template <int ST, int SIDE>
__device__ __forceinline__ float desc_cell_mean(const float* s_ri, const float* s_dx, const float* s_dy, int lane)
{
    constexpr int LAT = 21;
    float acc = 0.0f;
    if (lane < SIDE * SIDE * 3) {
        const int cell = lane / 3, ch = lane - cell * 3;
        const int ci = cell / SIDE, cj = cell - ci * SIDE;          // i outer (k), j inner (l): descriptors.rs:117-118
        const float* src = (ch == 0 ? s_ri : (ch == 1 ? s_dx : s_dy)) + (ci * ST) * LAT + cj * ST;
#pragma unroll
        for (int kk = 0; kk < ST; ++kk)
#pragma unroll
            for (int ll = 0; ll < ST; ++ll) acc += src[kk * LAT + ll];
    }
    return acc / (float)(ST * ST);
}

// The three grids sample the SAME lattice: sample (k, l) of any grid sits at
// (xf + (-l*si*scale + k*co*scale), yf + (l*co*scale + k*si*scale)) with integer k, l in [-10, 10] (the 3x3 grid
// of step 7 reaches +10, the other two stop at +9), so the 21 x 21 = 441 lattice values are gathered ONCE
// (7 rounds of 64 lanes, all loads in flight) and parked in the wave's LDS segment; the 4 + 9 + 16 = 29 cells
// are then summed concurrently, one lane per cell, each in the reference's (k outer, l inner) order.
constexpr int kDescWaves = 1;   // waves (keypoints) per block: one, so a block's 6 KB of LDS fits beside the scale-space
                                // stream's blocks, which fill most of a CU's LDS (four per block: 0.6 % slower end to end)
__global__ __launch_bounds__(64 * kDescWaves) void k_describe_fast(LevelTable T, const DescTables* __restrict__ desc_p,
                                                       const DevKp* __restrict__ in,
                                                       const uint32_t* __restrict__ n_in, uint32_t stride,
                                                       const uint32_t* __restrict__ perm,
                                                       akz_descriptor* __restrict__ out, uint32_t* __restrict__ flag)
{
    constexpr int LAT = 21, NS = LAT * LAT, NIT = (NS + 63) / 64, SMAX = 448;
    __shared__ float s_ri[kDescWaves][SMAX], s_dx[kDescWaves][SMAX], s_dy[kDescWaves][SMAX];
    __shared__ float s_val[kDescWaves][96];
    const DescTables& c_desc = *desc_p;
    const uint2 blk = xcd_block2(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
    const int frame = (int)blk.y;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t n = min(n_in[frame], stride);
    const uint32_t vi = blk.x * kDescWaves + wv;
    if (vi >= n) return;  // whole wave; no block-level barrier below
    const uint32_t ki = perm[(size_t)frame * stride + vi];  // spatially coherent visiting order
    const DevKp kp = in[(size_t)frame * stride + ki];
    const LevelDesc& L = T.L[kp.class_id];
    // get_mldb_descriptor, descriptors.rs:66-72
    const float ratio = (float)(1u << kp.octave);
    const float scale = roundf(0.5f * kp.size / ratio);
    const float xf = kp.x / ratio, yf = kp.y / ratio;
    const float co = akz_pm_cosf(kp.angle), si = akz_pm_sinf(kp.angle);
    const float* LT = L.Lt + (size_t)frame * L.fs;
    const float2* LXY = L.Lxy + (size_t)frame * L.fs;
    const int W = L.w, Hh = L.h;
    bool oob = false;
    int idx[NIT], canon[NIT];
    // consecutive lanes take consecutive lattice samples along the lattice axis whose image-space step is the more
    // HORIZONTAL one (k steps by scale * (co, si), l by scale * (-si, co)): the lanes of a quad then fall on the same
    // row and mostly the same cache line, which is what the texture addresser coalesces (wave-uniform choice)
    const bool k_fast = fabsf(co) > fabsf(si);
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int s = it * 64 + lane;
        const bool on = s < NS;
        const int qa = s / LAT, qb = s - qa * LAT;
        const int kq = k_fast ? qb : qa, lq = k_fast ? qa : qb;
        canon[it] = kq * LAT + lq;                       // position in the (k outer, l inner) lattice the sums walk
        const float kf = (float)(kq - 10), lf = (float)(lq - 10);
        // descriptors.rs:127-128, exact expression order
        float sample_y = yf + (lf * co * scale + kf * si * scale);
        float sample_x = xf + (-lf * si * scale + kf * co * scale);
        int y1 = sat_i32(roundf(sample_y));
        int x1 = sat_i32(roundf(sample_x));
        bool bad = x1 < 0 || x1 >= W || y1 < 0 || y1 >= Hh;
        oob |= on && bad;   // Error::SampleOutOfBounds in any grid drops the keypoint (descriptors.rs:28)
        idx[it] = (on && !bad) ? y1 * W + x1 : 0;
    }
    float ri[NIT];
    float2 dd[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        ri[it] = LT[idx[it]];
        dd[it] = LXY[idx[it]];
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int s = it * 64 + lane;
        float rry = dd[it].x * co + dd[it].y * si;     // descriptors.rs:151-152
        float rrx = -dd[it].x * si + dd[it].y * co;
        if (s < NS) {
            s_ri[wv][canon[it]] = ri[it];
            s_dx[wv][canon[it]] = rrx;
            s_dy[wv][canon[it]] = rry;
        }
    }
    oob = __any(oob);
    if (!oob) {
        // one lane per (cell, channel): 12 + 27 + 48 independent serial sums, each grid a pass with compile-time
        // loop bounds (one LDS read and one add per sample), in the reference's (k outer, l inner) order
        desc_cells<10, 2, 0>(s_ri[wv], s_dx[wv], s_dy[wv], s_val[wv], lane);
        desc_cells<7, 3, 12>(s_ri[wv], s_dx[wv], s_dy[wv], s_val[wv], lane);
        desc_cells<5, 4, 39>(s_ri[wv], s_dx[wv], s_dy[wv], s_val[wv], lane);
    }
    // mldb_binary_comparisons, descriptors.rs:181-202: bit b -> byte b>>3, position b&7 (LSB first)
    uint32_t byte = 0;
    if (!oob) {
        for (int t = 0; t < 8; ++t) {
            int b = lane * 8 + t;
            if (b < c_desc.n_bits) {
                float va = s_val[wv][c_desc.cmp_a[b]], vb = s_val[wv][c_desc.cmp_b[b]];
                byte |= (va > vb ? 1u : 0u) << t;
            }
        }
    }
    out[(size_t)frame * stride + ki].bytes[lane] = (uint8_t)byte;
    if (lane == 0) flag[(size_t)frame * stride + ki] = oob ? 0u : 1u;
}

// ---------------------------------------------------------------------------------------------
// A13 alone, one THREAD per keypoint: the sub-pixel fit needs nine determinant values the candidate list already
// carries.  The orientation (A14) moves to the descriptor kernel below, where its arithmetic runs in the shadow of
// the descriptor's gathers (k_refine with both is VALU-bound, k_describe_fast latency-bound: one after the other
// they cost the sum, fused the larger of the two).
__global__ __launch_bounds__(256) void k_refine_pos(LevelTable T, const DevKp* __restrict__ in,
                                                    const uint32_t* __restrict__ n_in, uint32_t stride,
                                                    DevKp* __restrict__ out, uint32_t* __restrict__ flag,
                                                    const float* __restrict__ cand_nb, uint32_t max_cand)
{
    const int frame = blockIdx.y;
    const uint32_t n = min(n_in[frame], stride);
    const uint32_t ki = blockIdx.x * 256 + threadIdx.x;
    if (ki >= n) return;
    DevKp kp = in[(size_t)frame * stride + ki];
    const bool keep = subpixel_fit(T, cand_nb, max_cand, frame, &kp);
    out[(size_t)frame * stride + ki] = kp;
    flag[(size_t)frame * stride + ki] = keep ? 1u : 0u;
}

// ---- helpers of k_orient_describe -------------------------------------------------------------------------------
// roundf(v) for the sample coordinates without roundf's compare-and-select sequence: for every f32 v >= 0,
// floor(v + 0.49999997f) == roundf(v) (0.49999997f = 0x3EFFFFFF, the largest f32 below 0.5: adding 0.5 itself would
// round 0.49999997 up to 1; tests/test_oracle_math.py walks every f32 of [2^-4, 2^25) against the definition), and for
// v < 0 the sum is negative exactly when v <= -0.5, i.e. when roundf(v) <= -1.
// `f32 as usize` of the rounded value (negatives and NaN -> 0): v_cvt_u32_f32 truncates toward zero and saturates.
__device__ __forceinline__ unsigned round_sat_u32(float v)
{
    unsigned r;
    asm("v_cvt_u32_f32 %0, %1" : "=v"(r) : "v"(v + 0.49999997f));
    return r;
}
// `f32 as isize` of the rounded value where only "inside [0, n)" matters: any v <= -0.5 gives a negative result (not
// necessarily roundf's), NaN gives 0 as Rust's cast does, the infinities saturate.
// (the caller has already added 0.49999997f: k_orient_describe does it for both coordinates in one packed add)
__device__ __forceinline__ int round_flr_i32_biased(float v_plus_bias)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(v_plus_bias));
    return r;
}

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_max_i32(int v)   // max(v, the DPP-selected lane's v); lanes without a source keep v
{
    return max(v, __builtin_amdgcn_update_dpp(v, v, CTRL, ROW_MASK, 0xf, false));
}

// Number of window end points below `ang` (OriTables::bnd, 128 sorted entries padded with +inf): 0..127.
__device__ __forceinline__ int ori_rank(const float* s_bnd, float ang)
{
    int r = 0;
#pragma unroll
    for (int step = 64; step > 0; step >>= 1) r += s_bnd[r + step - 1] < ang ? step : 0;
    return r;
}

// The angle of compute_main_orientation (scale_space_extrema.rs:242) is only ever COMPARED with the windows' end points,
// and evaluating it exactly (akz_pm_atan2f: f64, two divisions) for 109 samples per keypoint was a quarter of the
// kernel's instructions.  So: an f32 estimate (one v_rcp_f32, a degree-15 odd polynomial, tools/fit_atan.py) places the
// sample among the end points, and whenever the estimate lies within kOriEps = 8e-6 of an end point — or the operands are
// outside the range the estimate is good for, or anything is NaN — the exact expression decides instead.  The band is
// PROVEN wide enough, not sampled: |estimate - exact expression| <= 1.84e-6 for every admitted input
// (tools/ubench/atan_bound.c: the polynomial against atan over every f32 argument by exhaustion, 1.63e-7; v_rcp_f32's 1 ulp
// and the product's rounding, 1.8e-7; the three reflections' constants and roundings, 7.2e-7; the f32 roundings of the
// exact expression itself, 7.7e-7; tests/test_oracle_math.py runs it on the coefficients of THIS file, and the -m gpu
// suite checks the reciprocal's ulp on the device for every operand the path admits).  Both 0 and 2 pi are end points, so the
// wrap of rem_euclid is covered by the same band.  (0, +x): exactly 0 in the reference, and common (flat areas, vertical
// edges): taken without the fallback.  Returns the membership bits (bit = window).
constexpr float kOriEps = 8e-6f;
// Returns the sample's entry of OriTables::m_tab: 2 rank + (the angle IS end point `rank`).
__device__ __forceinline__ int ori_sample_entry(float ry, float rx, const float* s_bnd, bool* fell_back)
{
    const float ax = fabsf(rx), ay = fabsf(ry);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = mn * __builtin_amdgcn_rcpf(mx);
    const float s = t * t;
    float p = -0.004668773151934147f;
    p = __builtin_fmaf(p, s, 0.02416618913412094f);
    p = __builtin_fmaf(p, s, -0.0593671016395092f);
    p = __builtin_fmaf(p, s, 0.09906096756458282f);
    p = __builtin_fmaf(p, s, -0.14016585052013397f);
    p = __builtin_fmaf(p, s, 0.19969235360622406f);
    p = __builtin_fmaf(p, s, -0.33331960439682007f);
    p = __builtin_fmaf(p, s, 0.9999998807907104f);
    float a = t * p;
    a = ay > ax ? 1.57079637050628662109f - a : a;
    a = __builtin_signbit(rx) ? 3.14159274101257324219f - a : a;
    a = __builtin_signbit(ry) ? 6.28318548202514648438f - a : a;
    const bool zero_known = ry == 0.0f && __float_as_uint(rx) <= 0x7F800000u;   // x = +0 .. +inf (not -0, not NaN)
    float ang = zero_known ? 0.0f : a;
    int r = ori_rank(s_bnd, ang);
    float b1 = s_bnd[r];
    const float b0 = s_bnd[r > 0 ? r - 1 : 0];
    // (ax < 1e30 && ay < 1e30 rather than mx < 1e30: v_max_f32 drops a NaN operand)
    const bool sure = zero_known || (mx > 1e-30f && ax < 1e30f && ay < 1e30f && fabsf(ang - b1) > kOriEps && fabsf(ang - b0) > kOriEps);
    if (!sure) {
        ang = fast_atan2_equiv(ry, rx);
        r = ori_rank(s_bnd, ang);
        b1 = s_bnd[r];
    }
    if (fell_back) *fell_back = !sure;
    return 2 * r + (b1 == ang ? 1 : 0);
}

// A14 + A16 + A17 for the default pattern: main orientation (as in k_refine), then the descriptor (as in
// k_describe_fast), one wave per keypoint, four keypoints per block (the orientation tables are staged once per
// block).  The wave's LDS segment is used twice: weighted gradients of the 109 orientation samples, then the 441 lattice
// values of the descriptor.  The angle is written back into the keypoint list.
//
// Round 4 (the kernel is the largest VALU consumer of the pipeline — 1 900 instructions per keypoint before — and, behind
// that, a chain of dependent memory round trips: count -> permutation -> keypoint record -> sample offsets -> orientation
// samples -> ... -> lattice samples -> comparison tables -> store, with six waves per SIMD to hide it):
//   * window membership from an f32 estimate of the angle, the exact f64 expression only inside a band around the
//     windows' end points (ori_sample_entry);
//   * the 42 window sums run with the sample's membership bits AS the execution mask: sample k's table entry goes from
//     its owner lane to an SGPR (v_readlane), its 64-bit mask follows by scalar load from the 2 KB table, `s_mov exec` and
//     one v_pk_add_f32 add {Lx, Ly} in exactly the lanes (windows) that contain it — 2 VALU instructions per sample
//     instead of 5 (bit test, compare, two selects, add), and a sample outside a window is skipped as the reference skips it;
//   * the window maximum by DPP row operations;
//   * the descriptor lattice as 7 rounds of 3 rows x 21 columns (lane 63 idle): the lane's column term and the integer
//     division leave the loop; coordinates rounded by one add and v_cvt_flr_i32_f32 (round_flr_i32_biased);
//   * the per-lane tables (sample offsets, weights, comparison pairs) are requested before the wave's first wait, so no
//     round trip precedes the comparisons; the cell means overwrite the dead lattice planes and the membership table
//     is read by scalar loads: 21.7 KB of LDS per block, seven waves per SIMD instead of six (which
//     measures the same, 5.51 against 5.42 ms per 256 frames: the kernel is no longer waiting on round trips — VALU issue
//     ~50 %, LDS and the texture path ~30 % each, no unit saturated).
//   (Built and dropped: a wave walking 4 / 8 / 16 consecutive keypoints with the next keypoint's samples requested behind
//   the current lattice gather — 7.9 / 9.6 / 10.8 ms per 256 frames against 5.9: the registers the walk carries leave the
//   scheduler two LDS reads in flight; the keypoint records copied into visiting order and fetched by scalar loads together
//   with the count, before the barrier — 5.61 / 5.52 ms against 5.45 with the plain count -> permutation -> record chain:
//   with seven waves per SIMD those round trips are hidden already.  A per-wave LDS segment that is not 8-byte aligned
//   doubles the kernel's time: the +1 below.)
constexpr int kODWaves = 4;     // keypoints (waves) per block: 2 / 4 / 8 / 16 measure 1 332 / 1 288 / 1 372 / 1 633 us per 64 frames
constexpr int kODOcc = 7;       // waves per SIMD the register budget is held to
struct ODHead {          // what the kernel needs of one keypoint (wave-uniform)
    float xf, yf, scale;
    const float* LT;
    const float2* LXY;
    int W, Hh;
    uint32_t ki;         // the keypoint's slot in the response-sorted list (where angle, descriptor and flag go)
};
__global__ __launch_bounds__(64 * kODWaves, kODOcc) void k_orient_describe(LevelTable T, const OriTables* __restrict__ ori_p,
                                                                   const DescTables* __restrict__ desc_p,
                                                                   DevKp* __restrict__ kps,
                                                                   const uint32_t* __restrict__ n_in, uint32_t stride,
                                                                   const uint32_t* __restrict__ perm,
                                                                   akz_descriptor* __restrict__ out,
                                                                   uint32_t* __restrict__ flag, uint32_t* __restrict__ err)
{
    constexpr int LAT = 21, NIT = 7, SMAX = LAT * LAT;
    typedef float v2f __attribute__((ext_vector_type(2)));
    // LDS: the end points (512 B) + 4 x 5 296 B of lattice planes = 21 696 B, seven blocks (seven waves per SIMD) per CU.  The
    // cell means overwrite the planes once the last sum has read them; the membership table is read by scalar loads (below).
    __shared__ float s_bnd[128];
    __shared__ __attribute__((aligned(16))) float s_w[kODWaves][3 * SMAX + 1];     // (+ 1: every wave's segment 16-byte aligned)
    const OriTables& c_ori = *ori_p;
    const DescTables& c_desc = *desc_p;
    const uint2 blk = xcd_block2(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y);
    const int frame = (int)blk.y;
    // the grid covers the list's capacity: a block past the frame's count (two in five at 5 000 of 8 192) leaves before it
    // stages anything
    const uint32_t n = min(n_in[frame], stride);
    if (blk.x * kODWaves >= n) return;   // whole block
    if (threadIdx.x < 128) s_bnd[threadIdx.x] = c_ori.bnd[threadIdx.x];
    const uint2* __restrict__ m_tab = c_ori.m_tab;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t vi = blk.x * kODWaves + (uint32_t)wv;
    const size_t fbase = (size_t)frame * stride;
    __syncthreads();          // the only block-level barrier (the staged tables): waves are independent from here on
    if (vi >= n) return;  // whole wave
    const uint32_t ki = perm[fbase + vi];  // spatially coherent visiting order
    const DevKp kp = kps[fbase + ki];
    const bool on1 = lane + 64 < 109;
    const int i1 = on1 ? lane + 64 : 0;
    const float dj0 = (float)c_ori.dj[lane], di0 = (float)c_ori.di[lane], gw0 = c_ori.gw[lane];
    const float dj1 = (float)c_ori.dj[i1], di1 = (float)c_ori.di[i1], gw1 = c_ori.gw[i1];
    uint2 cmpa, cmpb;        // value indices compared for the lane's output byte (bits 8 lane .. 8 lane + 7)
    __builtin_memcpy(&cmpa, &c_desc.cmp_a[lane * 8], 8);
    __builtin_memcpy(&cmpb, &c_desc.cmp_b[lane * 8], 8);
    const int n_bits = c_desc.n_bits, n_win = c_ori.n_win;
    const bool on = lane < 63;
    const int line0 = lane / LAT, pos = lane - line0 * LAT;
    const float fpos = (float)(pos - 10);
    float2* s_r = reinterpret_cast<float2*>(s_w[wv]);             // [128] weighted {Lx, Ly} of every orientation sample
    float* s_ri = s_w[wv];
    float* s_dx = s_w[wv] + SMAX;
    float* s_dy = s_w[wv] + 2 * SMAX;
    float* s_val = s_w[wv];                                        // [87] the cell means, over the dead planes

    auto load_head = [&]() {
        ODHead h;
        h.ki = ki;
        const LevelDesc& L = T.L[kp.class_id];
        const float ratio = (float)(1u << kp.octave);
        h.xf = kp.x / ratio;
        h.yf = kp.y / ratio;
        h.scale = roundf(0.5f * kp.size / ratio);   // scale_space_extrema.rs:236 and descriptors.rs:69: the same value
        h.LT = L.Lt + (size_t)frame * L.fs;
        h.LXY = L.Lxy + (size_t)frame * L.fs;
        h.W = L.w;
        h.Hh = L.h;
        return h;
    };
    const ODHead cur = load_head();
    // the two orientation samples of this lane (scale_space_extrema.rs:236-241)
    unsigned iy0 = round_sat_u32(cur.yf + dj0 * cur.scale), ix0 = round_sat_u32(cur.xf + di0 * cur.scale);
    unsigned iy1 = round_sat_u32(cur.yf + dj1 * cur.scale), ix1 = round_sat_u32(cur.xf + di1 * cur.scale);
    const bool outside = ix0 >= (unsigned)cur.W || iy0 >= (unsigned)cur.Hh || ix1 >= (unsigned)cur.W || iy1 >= (unsigned)cur.Hh;
    ix0 = min(ix0, (unsigned)cur.W - 1u); iy0 = min(iy0, (unsigned)cur.Hh - 1u);
    ix1 = min(ix1, (unsigned)cur.W - 1u); iy1 = min(iy1, (unsigned)cur.Hh - 1u);
    const size_t o0 = (size_t)iy0 * cur.W + ix0, o1 = (size_t)iy1 * cur.W + ix1;
    if (outside) atomicOr(err, 8u);        // the reference would panic here
    const float2 smp0 = cur.LXY[o0], smp1 = cur.LXY[o1];
    // ---- compute_main_orientation, scale_space_extrema.rs:229-288 ----
    int ent0, ent1;                                                // m_tab entries of samples lane and 64 + lane
    {
        const float rx0 = gw0 * smp0.x, ry0 = gw0 * smp0.y;
        const float rx1 = gw1 * smp1.x, ry1 = gw1 * smp1.y;
        s_r[lane] = make_float2(rx0, ry0);
        s_r[lane + 64] = make_float2(rx1, ry1);
        // window membership of the samples (:261-287) from the end-point table (see k_refine)
        ent0 = 8 * ori_sample_entry(ry0, rx0, s_bnd, nullptr);       // (as byte offsets into the table)
        ent1 = 8 * ori_sample_entry(ry1, rx1, s_bnd, nullptr);
        if (!on1) ent1 = 8 * 256;
    }
    float angle;
    {
        // sums of the windows, lane <-> window, samples in the reference's order
        v2f sum = {0.0f, 0.0f};                       // {sum_x, sum_y}: one packed add per sample
        // (EXEC is rewritten inside the statements below and restored by them; every lane of the wave is live here — the only
        // exit above is taken by whole waves — so no lane the compiler holds inactive can be switched on.)
        // Four samples per step.  A sample's 42 membership bits reach an SGPR pair without crossing the vector ALU twice: its
        // table ENTRY travels (one v_readlane), the bits follow by scalar load from the 2 KB table (resident in the scalar
        // cache): tools/ubench/window_sum.hip prices a v_readlane at ~4.3 of the step's 18 SIMD cycles.
        auto m64 = [&](int k) {
            const uint32_t e = (uint32_t)__builtin_amdgcn_readlane(k < 64 ? ent0 : ent1, k & 63);      // byte offset of the entry
            const uint2 mk = *reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(m_tab) + e);
            return ((unsigned long long)mk.y << 32) | mk.x;
        };
        auto rv = [&](int k) {
            const float2 rk = s_r[k];
            return (v2f){rk.x, rk.y};
        };
#pragma unroll
        for (int k = 0; k + 4 <= 108; k += 4) {
            const unsigned long long m0 = m64(k), m1 = m64(k + 1), m2 = m64(k + 2), m3 = m64(k + 3);
            const v2f r0 = rv(k), r1 = rv(k + 1), r2 = rv(k + 2), r3 = rv(k + 3);
            unsigned long long saved;
            asm("s_mov_b64 %[sv], exec\n\t"
                "s_mov_b64 exec, %[m0]\n\tv_pk_add_f32 %[s], %[s], %[r0]\n\t"
                "s_mov_b64 exec, %[m1]\n\tv_pk_add_f32 %[s], %[s], %[r1]\n\t"
                "s_mov_b64 exec, %[m2]\n\tv_pk_add_f32 %[s], %[s], %[r2]\n\t"
                "s_mov_b64 exec, %[m3]\n\tv_pk_add_f32 %[s], %[s], %[r3]\n\t"
                "s_mov_b64 exec, %[sv]"
                : [s] "+v"(sum), [sv] "=&s"(saved)
                : [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2), [m3] "s"(m3), [r0] "v"(r0), [r1] "v"(r1), [r2] "v"(r2), [r3] "v"(r3));
        }
        {
            const unsigned long long m0 = m64(108);
            const v2f r0 = rv(108);
            unsigned long long saved;
            asm("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[m0]\n\tv_pk_add_f32 %[s], %[s], %[r0]\n\ts_mov_b64 exec, %[sv]"
                : [s] "+v"(sum), [sv] "=&s"(saved)
                : [m0] "s"(m0), [r0] "v"(r0));
        }
        const float sum_x = sum.x, sum_y = sum.y;
        const float val = sum_x * sum_x + sum_y * sum_y;
        // the serial loop keeps the FIRST window whose val exceeds every earlier one (a NaN never does).  val >= +0, so
        // its bit pattern orders as an integer; lanes beyond the windows and NaNs enter as -1
        const bool is_win = lane < n_win && val == val;
        const int vbits = is_win ? __float_as_int(val) : -1;
        int mr = vbits;
        mr = dpp_max_i32<0xB1>(mr);            // quad_perm [1,0,3,2]
        mr = dpp_max_i32<0x4E>(mr);            // quad_perm [2,3,0,1]
        mr = dpp_max_i32<0x141>(mr);           // row_half_mirror
        mr = dpp_max_i32<0x140>(mr);           // row_mirror: every lane of a row of 16 holds the row's maximum
        mr = dpp_max_i32<0x142, 0xa>(mr);      // row_bcast:15 into rows 1 and 3
        mr = dpp_max_i32<0x143, 0xc>(mr);      // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's maximum
        const int mbits = __builtin_amdgcn_readlane(mr, 63);
        const unsigned long long bal = __ballot(is_win && vbits == mbits);
        const int win = bal ? __ffsll((long long)bal) - 1 : 0;
        const float best_sx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sum_x), win));
        const float best_sy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sum_y), win));
        angle = (mbits > 0) ? fast_atan2_equiv(best_sy, best_sx) : 0.0f;
        if (lane == 0) kps[fbase + cur.ki].angle = angle;
    }
    // the segment changes hands: every LDS read above has returned before the writes below are issued
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- get_mldb_descriptor, descriptors.rs:66-72 (as k_describe_fast) ----
    const float co = akz_pm_cosf(angle), si = akz_pm_sinf(angle);
    const float scale = cur.scale, xf = cur.xf, yf = cur.yf;
    const int W = cur.W, Hh = cur.Hh;
    bool oob = false;
    int idx[NIT];
    // Lattice sample (k, l) sits at (xf + (-l*si*scale + k*co*scale), yf + (l*co*scale + k*si*scale)), descriptors.rs:127-128.
    // Consecutive lanes take consecutive samples along the lattice axis whose image-space step is the more HORIZONTAL
    // one (k steps by scale * (co, si), l by scale * (-si, co)): the lanes of a quad then fall on the same row and mostly
    // the same cache line (wave-uniform choice).  A round is 3 lines of 21 samples along that axis: the lane's position
    // on the line (its term of both sums) is fixed, the line advances by 3 per round.
    const bool k_fast = fabsf(co) > fabsf(si);
    // k_fast: k = pos, l = line:  y = yf + ((l*co)*scale + (k*si)*scale),  x = xf + (((-l)*si)*scale + (k*co)*scale)
    // else:   l = pos, k = line:  the same expressions with the roles swapped; a + b == b + a, (-l)*si == l*(-si)
    // both coordinates of a sample in one packed operation each ({x, y}: v_pk_mul_f32 / v_pk_add_f32 round each half as the
    // scalar instruction would)
    const v2f cxy = {k_fast ? -si : co, k_fast ? co : si};         // factors of the line number in {x, y}
    const v2f fix = {k_fast ? fpos * co * scale : -fpos * si * scale, k_fast ? fpos * si * scale : fpos * co * scale};
    const v2f base = {xf, yf}, scale2 = {scale, scale}, half_ulp = {0.49999997f, 0.49999997f};
    // position in the (k outer, l inner) lattice the sums walk
    const int canon0 = k_fast ? pos * LAT + line0 : lane;          // line0 * LAT + pos == lane
    const int cstep = k_fast ? 3 : 3 * LAT;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const float fl = (float)(line0 + 3 * it - 10);
        const v2f fl2 = {fl, fl};
        const v2f smp = (base + (fl2 * cxy * scale2 + fix)) + half_ulp;
        const int x1 = round_flr_i32_biased(smp.x), y1 = round_flr_i32_biased(smp.y);
        const bool bad = (unsigned)x1 >= (unsigned)W || (unsigned)y1 >= (unsigned)Hh;
        oob |= on && bad;   // Error::SampleOutOfBounds in any grid drops the keypoint (descriptors.rs:28)
        idx[it] = (on && !bad) ? y1 * W + x1 : 0;
    }
    float ri[NIT];
    float2 dd[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        ri[it] = cur.LT[idx[it]];
        dd[it] = cur.LXY[idx[it]];
    }
    const v2f rot_x = {co, -si}, rot_y = {si, co};
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        // descriptors.rs:151-152: rry = dx*co + dy*si, rrx = -dx*si + dy*co ((-dx)*si == dx*(-si))
        const v2f dx2 = {dd[it].x, dd[it].x}, dy2 = {dd[it].y, dd[it].y};
        const v2f rr = dx2 * rot_x + dy2 * rot_y;                          // {rry, rrx}
        if (on) {
            const int canon = canon0 + it * cstep;
            s_ri[canon] = ri[it];
            s_dx[canon] = rr.y;
            s_dy[canon] = rr.x;
        }
    }
    oob = __any(oob);
    if (!oob) {
        const float m2 = desc_cell_mean<10, 2>(s_ri, s_dx, s_dy, lane);
        const float m3 = desc_cell_mean<7, 3>(s_ri, s_dx, s_dy, lane);
        const float m4 = desc_cell_mean<5, 4>(s_ri, s_dx, s_dy, lane);
        // (a wave's LDS accesses execute in order: the sums above have read the planes before these stores land on them)
        if (lane < 12) s_val[lane] = m2;
        if (lane < 27) s_val[12 + lane] = m3;
        if (lane < 48) s_val[39 + lane] = m4;
    }
    // mldb_binary_comparisons, descriptors.rs:181-202: bit b -> byte b>>3, position b&7 (LSB first)
    uint32_t byte = 0;
    if (!oob) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t ia = ((t < 4 ? cmpa.x : cmpa.y) >> (8 * (t & 3))) & 0xFFu;
            const uint32_t ib = ((t < 4 ? cmpb.x : cmpb.y) >> (8 * (t & 3))) & 0xFFu;
            const float va = s_val[ia], vb = s_val[ib];
            byte |= (lane * 8 + t < n_bits && va > vb ? 1u : 0u) << t;
        }
    }
    out[fbase + cur.ki].bytes[lane] = (uint8_t)byte;
    if (lane == 0) flag[fbase + cur.ki] = oob ? 0u : 1u;
}

void build_level_table(akz_ctx* c, LevelTable* T)
{
    const AkzPlan& P = c->plan;
    AkzSet& S = c->S();
    T->n = (int)P.levels.size();
    uint32_t rows = 0;
    for (int i = 0; i < T->n; ++i) {
        const AkzLevel& L = P.levels[i];
        LevelDesc& d = T->L[i];
        d.Ldet = S.Ldet[i];
        d.Lt = S.Lt[i];
        d.Lxy = S.Lxy[i];
        d.w = L.w;
        d.h = L.h;
        d.fs = L.pixels();
        d.octave = L.octave;
        d.kp_size = L.kp_size;
        d.row_off = rows;
        rows += (uint32_t)L.h + 1u;
    }
    T->rows_total = rows;
}

}  // namespace

size_t akz_ori_table_bytes() { return sizeof(OriTables); }
size_t akz_desc_table_bytes() { return sizeof(DescTables); }


// ---------------------------------------------------------------------------------------------
// host-side constant tables
int32_t akz_upload_tables(akz_ctx* c)
{
    const akz_config& cfg = c->cfg;
    static const float GAUSS25[7][7] = {
        {0.02546481f, 0.02350698f, 0.01849125f, 0.01239505f, 0.00708017f, 0.00344629f, 0.00142946f},
        {0.02350698f, 0.02169968f, 0.01706957f, 0.01144208f, 0.00653582f, 0.00318132f, 0.00131956f},
        {0.01849125f, 0.01706957f, 0.01342740f, 0.00900066f, 0.00514126f, 0.00250252f, 0.00103800f},
        {0.01239505f, 0.01144208f, 0.00900066f, 0.00603332f, 0.00344629f, 0.00167749f, 0.00069579f},
        {0.00708017f, 0.00653582f, 0.00514126f, 0.00344629f, 0.00196855f, 0.00095820f, 0.00039744f},
        {0.00344629f, 0.00318132f, 0.00250252f, 0.00167749f, 0.00095820f, 0.00046640f, 0.00019346f},
        {0.00142946f, 0.00131956f, 0.00103800f, 0.00069579f, 0.00039744f, 0.00019346f, 0.00008024f},
    };
    static const int id[13] = {6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6};
    OriTables ot;
    memset(&ot, 0, sizeof(ot));
    int idx = 0;
    for (int j = -6; j <= 6; ++j)
        for (int i = -6; i <= 6; ++i)
            if (i * i + j * j < 36) {
                ot.di[idx] = (signed char)i;
                ot.dj[idx] = (signed char)j;
                ot.gw[idx] = GAUSS25[id[j + 6]][id[i + 6]];
                idx++;
            }
    if (idx != 109) return AKZ_E_INTERNAL;
    {
        const float PI_F = 3.14159274101257324219f;
        volatile float ang1 = 0.0f;  // volatile: keep the f32 accumulation literal
        int nw = 0;
        while (ang1 < 2.0f * PI_F && nw < 48) {
            ot.ang1[nw++] = ang1;
            ang1 = ang1 + 0.15f;
        }
        if (nw >= 48) return AKZ_E_INTERNAL;
        ot.n_win = nw;
        // end points of every window, 0 and 2 pi, sorted and distinct
        std::vector<float> b = {0.0f, 2.0f * PI_F};
        for (int wd = 0; wd < nw; ++wd) {
            volatile float a1 = ot.ang1[wd];
            volatile float a2 = (a1 + PI_F / 3.0f > 2.0f * PI_F) ? a1 - 5.0f * PI_F / 3.0f : a1 + PI_F / 3.0f;
            b.push_back((float)a1);
            b.push_back((float)a2);
        }
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        const int nb = (int)b.size();
        if (nb > 127) return AKZ_E_INTERNAL;
        auto mask_of = [&](float ang) {
            uint64_t m = 0;
            for (int wd = 0; wd < nw; ++wd) m |= (uint64_t)(ori_window_contains(ot.ang1[wd], ang) ? 1 : 0) << wd;
            return make_uint2((uint32_t)m, (uint32_t)(m >> 32));
        };
        for (int r = 0; r < 128; ++r) {
            ot.bnd[r] = r < nb ? b[r] : INFINITY;
            ot.m_eq[r] = r < nb ? mask_of(b[r]) : make_uint2(0u, 0u);
            // any angle strictly between b[r-1] and b[r] (membership is constant there): the float above b[r-1],
            // or one below b[0]; above the last end point (>= 2 pi) nothing is a member
            float probe = r == 0 ? -1.0f : (r <= nb ? nextafterf(b[r - 1], INFINITY) : INFINITY);
            ot.m_open[r] = (r <= nb && !(r < nb && probe >= b[r])) ? mask_of(probe) : make_uint2(0u, 0u);
            ot.m_tab[2 * r] = ot.m_open[r];
            ot.m_tab[2 * r + 1] = ot.m_eq[r];
        }
        ot.m_tab[256] = make_uint2(0u, 0u);
        // self-check of the table against the predicate at every end point and the floats next to it
        auto lookup = [&](float ang) {
            int r = 0;
            for (int step = 64; step > 0; step >>= 1) r += ot.bnd[r + step - 1] < ang ? step : 0;
            return (r < 128 && ot.bnd[r & 127] == ang) ? ot.m_eq[r & 127] : ot.m_open[r & 127];
        };
        for (int r = 0; r < nb; ++r)
            for (float ang : {nextafterf(b[r], -INFINITY), b[r], nextafterf(b[r], INFINITY)}) {
                const uint2 want = mask_of(ang), got = lookup(ang);
                if (want.x != got.x || want.y != got.y) return AKZ_E_INTERNAL;
            }
    }
    AKZ_HIP(hipMemcpy(c->d_ori, &ot, sizeof(ot), hipMemcpyHostToDevice));

    DescTables dt;
    memset(&dt, 0, sizeof(dt));
    const int pattern = (int)cfg.descriptor_pattern_size;
    const int nch = (int)cfg.descriptor_channels;
    if (nch < 1 || nch > 3 || pattern < 1 || pattern > 100) return AKZ_E_INVALID;
    const float size_mult[3] = {1.0f, 2.0f / 3.0f, 1.0f / 2.0f};
    int cell = 0, vpos_total = 0, bit = 0;
    for (int lvl = 0; lvl < 3; ++lvl) {
        int val_count = (lvl + 2) * (lvl + 2);
        float fs = ceilf((float)pattern * size_mult[lvl]);
        int step = (int)fs;
        if (step < 1) return AKZ_E_INVALID;
        int cells_here = 0;
        // the value array is REUSED per grid in the reference (values[valuepos] restarts at 0); we keep one
        // private segment per grid instead, which the comparison table indexes accordingly.
        for (int i = -pattern; i < pattern; i += step)
            for (int j = -pattern; j < pattern; j += step) {
                if (cell >= 32) return AKZ_E_INVALID;
                dt.ci[cell] = (signed char)i;
                dt.cj[cell] = (signed char)j;
                dt.step[cell] = (unsigned char)step;
                dt.vbase[cell] = (unsigned char)(vpos_total + cells_here * nch);
                cell++;
                cells_here++;
            }
        if (cells_here != val_count) return AKZ_E_INVALID;  // the reference assumes (lvl+2)^2 cells
        for (int pos = 0; pos < nch; ++pos)
            for (int i = 0; i < val_count; ++i)
                for (int j = i + 1; j < val_count; ++j) {
                    if (bit >= 512) return AKZ_E_INVALID;
                    dt.cmp_a[bit] = (unsigned char)(vpos_total + nch * i + pos);
                    dt.cmp_b[bit] = (unsigned char)(vpos_total + nch * j + pos);
                    bit++;
                }
        vpos_total += val_count * nch;
    }
    dt.n_cells = cell;
    dt.nch = nch;
    dt.n_bits = bit;
    if (vpos_total > 96) return AKZ_E_INVALID;
    AKZ_HIP(hipMemcpy(c->d_desc, &dt, sizeof(dt), hipMemcpyHostToDevice));
    return AKZ_OK;
}

// ---- the keypoint stage's host code: route, then launch ---------------------------------------------------------------
// The templated kernels, named once in the order the code object has carried them since they were written: implicit
// instantiations are emitted in the order of their first mention (rs_ransac.hip's kKernelOrder), so the host code below can
// be edited without reordering the device code.
[[maybe_unused]] static const void* const kKernelOrder[] = {
    (const void*)k_sup_resolve<true>,        (const void*)k_sup_resolve<false>,      (const void*)k_compact<false>,
    (const void*)k_rank_sort<RANK_RESPONSE>, (const void*)k_rank_sort<RANK_SPATIAL>, (const void*)k_compact<true>};

// Every decision of one call.  route_keypoints makes them and enqueues nothing; the phase functions below launch what the
// route says and decide nothing.
enum VisitOrder {
    VISIT_STORED,    // non-default pattern: k_describe walks the list as stored
    VISIT_RASTER,    // the pre-sort order, written by the response sort
    VISIT_RANK,      // k_rank_sort<RANK_SPATIAL>
    VISIT_TILE,      // k_tile_order
    VISIT_BITONIC,   // k_spatial_order
};
struct KeypointRoute {
    // A12b, first pass
    bool sup_parallel;       // k_cand_rows, k_sup_adj, k_sup_resolve first; k_suppress then takes only the frames they flag
    bool resolve_chunked;    // k_sup_resolve<true>: the chunks of a frame on workgroups of their own
    dim3 grid_adj, grid_resolve;
    bool big_pass;           // k_suppress_big after k_suppress
    bool clear_big_flag;     // d_big_flag is cleared on its own (the parallel path clears it together with its flags)
    // A12b, second pass
    uint32_t kb, yr_stride;  // blocks of 256 cache entries, 64-entry chunks per frame
    // A13 + A14
    uint32_t kw;             // blocks of four waves, one keypoint per wave
    bool fast_desc;          // the default pattern: k_describe_fast / k_orient_describe and a visiting order
    bool orient_in_desc;     // k_refine_pos here, the orientation in k_orient_describe
    // A15
    uint32_t maxf;
    bool rank_sorts;         // k_rank_sort, not one block per frame
    bool raster_visit;
    dim3 grid_rank;
    uint32_t np2, lds_keys;  // padded list length of the largest frame; keys the bitonic orders hold in LDS
    size_t sort_lds;
    // A16 + A17
    VisitOrder order;
    uint32_t nbuckets;       // (level, tile) buckets of a frame: VISIT_TILE and VISIT_BITONIC
    size_t order_lds;
};

static KeypointRoute route_keypoints(const akz_ctx* c, int n, const LevelTable& T)
{
    KeypointRoute R = {};
    R.sup_parallel = c->sup_parallel;
    R.resolve_chunked = n <= 16;
    const uint32_t adj_blocks = (uint32_t)akz_div_up((int)c->sup_cap, 256);
    R.grid_adj = dim3(n > 16 && adj_blocks > 48u ? 48u : adj_blocks, n);
    R.grid_resolve = R.resolve_chunked ? dim3(akz_div_up((int)c->sup_cap, 1024), n) : dim3(1, n);
    // contexts created for more than kActCap keypoints per frame: a frame whose active list outgrows the LDS starts over in
    // k_suppress_big (its list: d_big_act, max_kp entries per frame)
    R.big_pass = c->max_kp > (uint32_t)kActCap;
    R.clear_big_flag = R.big_pass && !R.sup_parallel;
    R.kb = (uint32_t)akz_div_up((int)c->max_kp, 256);
    R.yr_stride = (uint32_t)akz_div_up((int)c->max_kp, 64);
    R.kw = (uint32_t)akz_div_up((int)c->max_kp, 4);
    // default pattern: the orientation is computed by the descriptor kernel (k_orient_describe); the refinement does only the
    // fit (not with the parity taps on: akz_debug_get_keypoints stage 1 is the list after refinement AND orientation)
    R.fast_desc = c->cfg.descriptor_pattern_size == 10 && c->cfg.descriptor_channels == 3;
    R.orient_in_desc = R.fast_desc && !c->keep_all;
    R.maxf = c->cfg.maximum_features > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)c->cfg.maximum_features;
    // few frames: the chip-wide rank sort; many: one block per frame, where the networks cost less than the n^2 comparisons
    // (74 vs 190 us per 64 frames of ~5 000 keypoints; a single 1080p frame: 154 -> ~20 us per sort the other way)
    R.rank_sorts = n <= 8;
    // Visiting order of the descriptor stage.  The response-sorted list is spatially random; the list BEFORE the sort is
    // in cache order (level-major, close to raster), and the sort knows where it sent every element — so when nothing is
    // truncated the descriptor kernel can walk the pre-sort order for free.  The (level, 32-px tile) order of
    // k_spatial_order is better for the gathers (84 vs 111 MB of HBM traffic per frame; 1 632 vs 1 708 us per 64 frames)
    // and costs a second sort (153 us).  A few-frame call, where every launch is on the critical path, takes the free
    // order; a batch takes the tile order (in the pipeline its sort hides and the lower traffic shows: 7 353-7 372 vs
    // 7 301-7 321 frames/s).
    R.raster_visit = R.rank_sorts && R.maxf >= c->max_kp;
    R.grid_rank = dim3((uint32_t)akz_div_up((int)c->max_kp, kRankI), n);
    R.np2 = 1;
    while (R.np2 < c->max_kp) R.np2 <<= 1;
    R.lds_keys = R.np2 < kAkzLdsSortKeys ? R.np2 : kAkzLdsSortKeys;   // longer lists: global key scratch
    R.sort_lds = R.rank_sorts ? 0 : std::max<size_t>(sizeof(unsigned long long) * R.lds_keys, kRadixSortLdsBytes);
    R.order = !R.fast_desc ? VISIT_STORED : R.raster_visit ? VISIT_RASTER : R.rank_sorts ? VISIT_RANK : VISIT_TILE;
    if (R.order == VISIT_TILE) {
        for (int e = 0; e < T.n; ++e)
            R.nbuckets += (((uint32_t)(T.L[e].w - 1) >> c->desc_tile_shift) + 1u) * (((uint32_t)(T.L[e].h - 1) >> c->desc_tile_shift) + 1u);
        // the counting sort while its buckets fit the LDS, the bitonic network over (level, tile, index) keys beyond
        if (R.nbuckets > kTileOrderMaxBuckets) R.order = VISIT_BITONIC;
        R.order_lds = R.order == VISIT_TILE ? sizeof(uint32_t) * R.nbuckets : sizeof(unsigned long long) * R.lds_keys;
    }
    return R;
}

// Hand over to the keypoint stream: everything after this is latency-bound per-frame work that overlaps the next
// micro-batch's scale space.
static int32_t kp_hand_over(akz_ctx* c)
{
    AKZ_HIP(hipEventRecord(c->ev_ss_done[c->cur], c->stream));
    AKZ_HIP(hipStreamWaitEvent(c->stream_kp, c->ev_ss_done[c->cur], 0));
    return AKZ_OK;
}

static int32_t kp_close(akz_ctx* c)
{
    AKZ_HIP(hipEventRecord(c->ev_kp_done[c->cur], c->stream_kp));
    c->kp_pending[c->cur] = true;
    return AKZ_OK;
}

// A12b, first pass
static int32_t kp_suppress(akz_ctx* c, int n, const LevelTable& T, const KeypointRoute& R)
{
    AkzSet& S = c->S();
    hipStream_t s = c->stream_kp;
    if (R.sup_parallel) {
        // the fallback flags sit directly before the scratch, whose first words are the chunk flags, the reverse-list
        // counters and the replaced marks
        AKZ_HIP(hipMemsetAsync(S.d_sup_flag, 0, (size_t)((char*)S.d_sup - (char*)S.d_sup_flag) +
                                                    sizeof(uint32_t) * sup_zero_words(c->sup_cap, (uint32_t)n), s));
        hipLaunchKernelGGL(k_cand_rows, dim3(T.n, n), dim3(1024), 0, s, T, S.d_ncand, S.d_cand, c->max_cand, S.d_cand_rows);
        AKZ_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sup_adj, R.grid_adj, dim3(256), 0, s, T, S.d_ncand, S.d_cand, c->max_cand, S.d_sup, c->sup_cap,
                           S.d_sup_flag, (const uint32_t*)S.d_cand_rows);
        AKZ_LAUNCH_CHECK();
        if (R.resolve_chunked)
            hipLaunchKernelGGL((k_sup_resolve<true>), R.grid_resolve, dim3(1024), 0, s, T, S.d_ncand, S.d_cand, c->max_cand, S.d_sup,
                               c->sup_cap, S.d_sup_flag, S.d_cache, c->max_kp, S.d_ncache, c->d_err, S.d_lvl_slot);
        else
            hipLaunchKernelGGL((k_sup_resolve<false>), R.grid_resolve, dim3(1024), 0, s, T, S.d_ncand, S.d_cand, c->max_cand, S.d_sup,
                               c->sup_cap, S.d_sup_flag, S.d_cache, c->max_kp, S.d_ncache, c->d_err, S.d_lvl_slot);
        AKZ_LAUNCH_CHECK();
    }
    if (R.clear_big_flag) AKZ_HIP(hipMemsetAsync(S.d_big_flag, 0, sizeof(uint32_t) * (size_t)n, s));
    hipLaunchKernelGGL(k_suppress, dim3(n), dim3(64), sizeof(ActEntry) * kActCap, s, T, S.d_ncand, S.d_cand, c->max_cand, S.d_cache,
                       c->max_kp, S.d_ncache, c->d_err, R.sup_parallel ? (const uint32_t*)S.d_sup_flag : (const uint32_t*)nullptr,
                       S.d_lvl_slot, R.big_pass ? S.d_big_flag : (uint32_t*)nullptr);
    AKZ_LAUNCH_CHECK();
    if (R.big_pass) {
        hipLaunchKernelGGL(k_suppress_big, dim3(n), dim3(64), 0, s, T, S.d_ncand, S.d_cand, c->max_cand, S.d_cache, c->max_kp,
                           S.d_ncache, c->d_err, (const uint32_t*)S.d_big_flag, S.d_lvl_slot,
                           reinterpret_cast<ActEntry*>(S.d_big_act), c->max_kp);
        AKZ_LAUNCH_CHECK();
    }
    return AKZ_OK;
}

// A12b, second pass: cache -> d_kp_a
static int32_t kp_filter_upper(akz_ctx* c, int n, const LevelTable& T, const KeypointRoute& R)
{
    AkzSet& S = c->S();
    hipStream_t s = c->stream_kp;
    float2* const yr_tab = reinterpret_cast<float2*>(S.d_chunk_yr);
    hipLaunchKernelGGL(k_chunk_yrange, dim3((uint32_t)akz_div_up((int)R.yr_stride, 4), n), dim3(256), 0, s, S.d_cache, c->max_kp,
                       S.d_ncache, yr_tab, R.yr_stride);
    AKZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_filter_upper, dim3(R.kb, n), dim3(256), sizeof(float2) * (size_t)R.yr_stride, s, S.d_cache, c->max_kp,
                       S.d_ncache, (const uint32_t*)S.d_lvl_slot, T.n, (const float2*)yr_tab, R.yr_stride, S.d_flag_b);
    AKZ_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_compact<false>), dim3(n), dim3(1024), 0, s, S.d_cache, (const akz_descriptor*)nullptr,
                       S.d_flag_b, S.d_ncache, c->max_kp, S.d_kp_a, (akz_descriptor*)nullptr, c->max_kp, S.d_n_a,
                       c->d_err, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    AKZ_LAUNCH_CHECK();
    return AKZ_OK;
}

// A13 + A14: d_kp_a -> d_kp_c
static int32_t kp_refine(akz_ctx* c, int n, const LevelTable& T, const KeypointRoute& R)
{
    AkzSet& S = c->S();
    hipStream_t s = c->stream_kp;
    akz_timer_begin(c, AKZ_T_REFINE, s);
    if (R.orient_in_desc)
        hipLaunchKernelGGL(k_refine_pos, dim3(R.kb, n), dim3(256), 0, s, T, S.d_kp_a, S.d_n_a, c->max_kp, S.d_kp_b, S.d_flag_b,
                           (const float*)S.d_cand_nb, c->max_cand);
    else
        hipLaunchKernelGGL(k_refine, dim3(R.kw, n), dim3(256), 0, s, T, (const OriTables*)c->d_ori, S.d_kp_a, S.d_n_a, c->max_kp,
                           S.d_kp_b, S.d_flag_b, c->d_err, (const float*)S.d_cand_nb, c->max_cand);
    AKZ_LAUNCH_CHECK();
    akz_timer_end(c, AKZ_T_REFINE, s, 1, (uint64_t)n);
    hipLaunchKernelGGL((k_compact<false>), dim3(n), dim3(1024), 0, s, S.d_kp_b, (const akz_descriptor*)nullptr,
                       S.d_flag_b, S.d_n_a, c->max_kp, S.d_kp_c, (akz_descriptor*)nullptr, c->max_kp, S.d_n_c,
                       c->d_err, (const uint32_t*)nullptr, (uint32_t*)nullptr);
    AKZ_LAUNCH_CHECK();
    return AKZ_OK;
}

// A15: d_kp_c -> d_kp_d
static int32_t kp_response_sort(akz_ctx* c, int n, const KeypointRoute& R)
{
    AkzSet& S = c->S();
    hipStream_t s = c->stream_kp;
    uint32_t* const perm = R.raster_visit ? S.d_perm : (uint32_t*)nullptr;
    if (R.rank_sorts)
        hipLaunchKernelGGL((k_rank_sort<RANK_RESPONSE>), R.grid_rank, dim3(256), 0, s, S.d_kp_c, S.d_n_c, c->max_kp, R.maxf, 0,
                           S.d_kp_d, S.d_n_d, perm);
    else
        hipLaunchKernelGGL(k_sort, dim3(n), dim3(1024), R.sort_lds, s, S.d_kp_c, S.d_n_c, c->max_kp, R.maxf, S.d_kp_d, S.d_n_d,
                           S.d_keys_kp, R.np2, R.lds_keys, perm);
    AKZ_LAUNCH_CHECK();
    return AKZ_OK;
}

// the order in which the descriptor kernel visits d_kp_d: d_perm
static int32_t kp_visit_order(akz_ctx* c, int n, const LevelTable& T, const KeypointRoute& R)
{
    AkzSet& S = c->S();
    hipStream_t s = c->stream_kp;
    switch (R.order) {
    case VISIT_STORED:
    case VISIT_RASTER: return AKZ_OK;
    case VISIT_RANK:
        hipLaunchKernelGGL((k_rank_sort<RANK_SPATIAL>), R.grid_rank, dim3(256), 0, s, S.d_kp_d, S.d_n_d, c->max_kp, 0u,
                           c->desc_tile_shift, (DevKp*)nullptr, (uint32_t*)nullptr, S.d_perm);
        break;
    case VISIT_TILE:
        hipLaunchKernelGGL(k_tile_order, dim3(n), dim3(1024), R.order_lds, s, T, S.d_kp_d, S.d_n_d, c->max_kp, S.d_perm,
                           c->desc_tile_shift);
        break;
    case VISIT_BITONIC:
        hipLaunchKernelGGL(k_spatial_order, dim3(n), dim3(1024), R.order_lds, s, T, S.d_kp_d, S.d_n_d, c->max_kp, S.d_perm,
                           c->desc_tile_shift, S.d_keys_kp, R.np2, R.lds_keys);
        break;
    }
    AKZ_LAUNCH_CHECK();
    return AKZ_OK;
}

// A16 + A17: descriptors of d_kp_d -> d_desc_tmp
static int32_t kp_describe(akz_ctx* c, int n, const LevelTable& T, const KeypointRoute& R)
{
    AkzSet& S = c->S();
    hipStream_t s = c->stream_kp;
    if (R.orient_in_desc) {
        akz_timer_begin(c, AKZ_T_ORIENT_DESCRIBE_K, s);
        AKZ_LAUNCH(k_orient_describe, dim3(((uint32_t)akz_div_up((int)c->max_kp, kODWaves) + 7u) & ~7u, n), dim3(64 * kODWaves), 0, s, T,
                   (const OriTables*)c->d_ori, (const DescTables*)c->d_desc, S.d_kp_d, S.d_n_d, c->max_kp,
                   S.d_perm, S.d_desc_tmp, S.d_flag_d, c->d_err);
        akz_timer_end(c, AKZ_T_ORIENT_DESCRIBE_K, s, 1, (uint64_t)n);
    } else if (R.fast_desc)
        hipLaunchKernelGGL(k_describe_fast, dim3((uint32_t)akz_div_up((int)c->max_kp, kDescWaves), n), dim3(64 * kDescWaves), 0, s, T,
                           (const DescTables*)c->d_desc, S.d_kp_d, S.d_n_d, c->max_kp, S.d_perm, S.d_desc_tmp, S.d_flag_d);
    else
        hipLaunchKernelGGL(k_describe, dim3(R.kw, n), dim3(256), 0, s, T, (const DescTables*)c->d_desc, S.d_kp_d, S.d_n_d, c->max_kp,
                           S.d_desc_tmp, S.d_flag_d);
    AKZ_LAUNCH_CHECK();
    return AKZ_OK;
}

// final compaction into the caller's arrays, and the event the next user of this buffer set waits for
static int32_t kp_finish(akz_ctx* c, int n, DevKp* d_kps, akz_descriptor* d_descs, uint32_t cap_per_img, uint32_t* d_n_out,
                         uint32_t* h_err_copy)
{
    AkzSet& S = c->S();
    hipLaunchKernelGGL((k_compact<true>), dim3(n), dim3(1024), 0, c->stream_kp, S.d_kp_d, S.d_desc_tmp, S.d_flag_d, S.d_n_d,
                       c->max_kp, d_kps, d_descs, cap_per_img, d_n_out, (uint32_t*)nullptr, (const uint32_t*)c->d_err, h_err_copy);
    AKZ_LAUNCH_CHECK();
    return kp_close(c);
}

int32_t akz_run_keypoints(akz_ctx* c, int n, DevKp* d_kps, akz_descriptor* d_descs, uint32_t cap_per_img,
                          uint32_t* d_n_out, uint32_t* h_err_copy)
{
    AkzTimerScope timer_scope(c);
    LevelTable T;
    if ((int)c->plan.levels.size() > kMaxLevels) return AKZ_E_INVALID;
    build_level_table(c, &T);
    if (T.n == 0) {
        // (candidate detection streams Ldet on the scale-space stream; with no level there is nothing for the other one to do)
        AKZ_HIP(hipMemsetAsync(d_n_out, 0, sizeof(uint32_t) * n, c->stream));
        AKZ_TRY(kp_hand_over(c));
        return kp_close(c);
    }
    const KeypointRoute R = route_keypoints(c, n, T);
    AKZ_TRY(kp_hand_over(c));
    AKZ_TRY(kp_suppress(c, n, T, R));
    AKZ_TRY(kp_filter_upper(c, n, T, R));
    AKZ_TRY(kp_refine(c, n, T, R));
    AKZ_TRY(kp_response_sort(c, n, R));
    akz_timer_begin(c, AKZ_T_DESCRIBE, c->stream_kp);
    AKZ_TRY(kp_visit_order(c, n, T, R));
    AKZ_TRY(kp_describe(c, n, T, R));
    akz_timer_end(c, AKZ_T_DESCRIBE, c->stream_kp, 1, (uint64_t)n);
    return kp_finish(c, n, d_kps, d_descs, cap_per_img, d_n_out, h_err_copy);
}

// ---- parity tap: the transcendentals of the orientation / descriptor kernels as the DEVICE evaluates them ----
// (compute_main_orientation's atan2, scale_space_extrema.rs:242; get_mldb_descriptor's cos / sin, descriptors.rs:70-71)
__global__ __launch_bounds__(256) void k_debug_portable_math(int which, const float* __restrict__ x, const float* __restrict__ y,
                                                             uint32_t n, float* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = which == 0 ? akz_pm_atan2f(y[i], x[i]) : (which == 1 ? akz_pm_sinf(x[i]) : akz_pm_cosf(x[i]));
}

extern "C" int32_t akz_debug_portable_math(akz_ctx* c, int32_t which, const float* x, const float* y, uint32_t n, float* out)
{
    return akz_guard([&]() -> int32_t {
        if (!c || !x || !out || which < 0 || which > 2 || (which == 0 && !y) || n == 0) return AKZ_E_INVALID;
        AKZ_HIP(hipSetDevice(c->device));
        float *dx = nullptr, *dy = nullptr, *dout = nullptr;
        AKZ_HIP(hipMalloc(&dx, sizeof(float) * n));
        AKZ_HIP(hipMalloc(&dy, sizeof(float) * n));
        AKZ_HIP(hipMalloc(&dout, sizeof(float) * n));
        AKZ_HIP(hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice));
        AKZ_HIP(hipMemcpy(dy, which == 0 ? y : x, sizeof(float) * n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_debug_portable_math, dim3((n + 255) / 256), dim3(256), 0, c->stream, which, dx, dy, n, dout);
        AKZ_LAUNCH_CHECK();
        AKZ_HIP(hipStreamSynchronize(c->stream));
        AKZ_HIP(hipMemcpy(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost));
        hipFree(dx); hipFree(dy); hipFree(dout);
        return AKZ_OK;
    });
}

// ---- the specification the angle estimate's error bound leans on, checked on the part itself ----
// v_rcp_f32 is specified to 1 ulp; tools/ubench/atan_bound.c (the bound behind kOriEps) uses exactly that.  This walks every
// f32 of [lo_bits, hi_bits] (bit patterns of positive floats), compares the instruction with 1 / x in f64 and returns the
// largest error in ulps of the correctly rounded quotient.
__global__ __launch_bounds__(256) void k_debug_rcp_error(uint32_t lo_bits, uint32_t hi_bits, unsigned long long* __restrict__ worst)
{
    double w = 0.0;
    const unsigned long long total = (unsigned long long)hi_bits - lo_bits + 1ull, stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < total; i += stride) {
        const float x = __uint_as_float(lo_bits + (uint32_t)i);
        const double exact = 1.0 / (double)x;
        const float r = __builtin_amdgcn_rcpf(x);
        int e;
        (void)frexp(exact, &e);                                   // exact = m 2^e, m in [0.5, 1): ulp of its f32 = 2^(e - 24)
        const double err = fabs((double)r - exact) * ldexp(1.0, 24 - e);
        w = err > w ? err : w;
    }
    // non-negative doubles order like their bit patterns
    atomicMax(worst, (unsigned long long)__double_as_longlong(w));
}

extern "C" int32_t akz_debug_rcp_error(akz_ctx* c, uint32_t lo_bits, uint32_t hi_bits, double* max_ulps)
{
    return akz_guard([&]() -> int32_t {
        if (!c || !max_ulps || lo_bits > hi_bits || hi_bits >= 0x7F800000u || lo_bits < 0x00800000u) return AKZ_E_INVALID;
        AKZ_HIP(hipSetDevice(c->device));
        unsigned long long* d = nullptr;
        AKZ_HIP(hipMalloc(&d, sizeof(*d)));
        int32_t rc = AKZ_OK;
        unsigned long long bits = 0;
        if (hipMemsetAsync(d, 0, sizeof(*d), c->stream) != hipSuccess) rc = AKZ_E_HIP;
        if (rc == AKZ_OK) {
            hipLaunchKernelGGL(k_debug_rcp_error, dim3(4096), dim3(256), 0, c->stream, lo_bits, hi_bits, d);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
                hipMemcpy(&bits, d, sizeof(bits), hipMemcpyDeviceToHost) != hipSuccess)
                rc = AKZ_E_HIP;
        }
        (void)hipFree(d);
        if (rc == AKZ_OK) memcpy(max_ulps, &bits, sizeof(bits));
        return rc;
    });
}

// ---- parity tap: the orientation samples' window membership, both ways ----
// fast[i]: ori_sample_entry + the table (the kernel's path: f32 estimate, exact expression inside the band); exact[i]: the exact
// expression alone; fell[i]: 1 where the band sent the sample to the exact expression.
__global__ __launch_bounds__(256) void k_debug_ori_masks(const OriTables* __restrict__ ori_p, const float* __restrict__ x,
                                                         const float* __restrict__ y, uint32_t n, uint2* __restrict__ fast,
                                                         uint2* __restrict__ exact, uint32_t* __restrict__ fell)
{
    __shared__ float s_bnd[128];
    if (threadIdx.x < 128) s_bnd[threadIdx.x] = ori_p->bnd[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool fb = false;
    fast[i] = ori_p->m_tab[ori_sample_entry(y[i], x[i], s_bnd, &fb)];
    fell[i] = fb ? 1u : 0u;
    const float ang = fast_atan2_equiv(y[i], x[i]);
    const int r = ori_rank(s_bnd, ang);
    exact[i] = s_bnd[r] == ang ? ori_p->m_eq[r] : ori_p->m_open[r];
}

extern "C" int32_t akz_debug_orientation_masks(akz_ctx* c, const float* x, const float* y, uint32_t n, uint64_t* fast,
                                               uint64_t* exact, uint32_t* fell_back)
{
    return akz_guard([&]() -> int32_t {
        if (!c || !x || !y || !fast || !exact || !fell_back || n == 0) return AKZ_E_INVALID;
        AKZ_HIP(hipSetDevice(c->device));
        float *dx = nullptr, *dy = nullptr;
        uint2 *df = nullptr, *de = nullptr;
        uint32_t* dfl = nullptr;
        int32_t rc = AKZ_OK;
        if (hipMalloc(&dx, sizeof(float) * n) != hipSuccess || hipMalloc(&dy, sizeof(float) * n) != hipSuccess ||
            hipMalloc(&df, sizeof(uint2) * n) != hipSuccess || hipMalloc(&de, sizeof(uint2) * n) != hipSuccess ||
            hipMalloc(&dfl, sizeof(uint32_t) * n) != hipSuccess) {
            rc = AKZ_E_HIP;
        } else if (hipMemcpy(dx, x, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess ||
                   hipMemcpy(dy, y, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess) {
            rc = AKZ_E_HIP;
        } else {
            hipLaunchKernelGGL(k_debug_ori_masks, dim3((n + 255) / 256), dim3(256), 0, c->stream, (const OriTables*)c->d_ori, dx, dy, n,
                               df, de, dfl);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
                hipMemcpy(fast, df, sizeof(uint2) * n, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(exact, de, sizeof(uint2) * n, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(fell_back, dfl, sizeof(uint32_t) * n, hipMemcpyDeviceToHost) != hipSuccess)
                rc = AKZ_E_HIP;
        }
        (void)hipFree(dx); (void)hipFree(dy); (void)hipFree(df); (void)hipFree(de); (void)hipFree(dfl);
        return rc;
    });
}
