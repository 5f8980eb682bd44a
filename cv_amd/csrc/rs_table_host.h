// rs_table_host.h — what the entry points of the observation-table stages (rs_landmark_table.hip, rs_bootstrap_table.hip,
// rs_reconstruction_merge.hip, rs_repack.hip, rs_export.hip, rs_observation_filter.hip) decide on the host before they
// enqueue anything: may two ranges share a byte, is a view list one of distinct blocks, where does a region of the scratch
// begin.  Host code only (no HIP, nothing is enqueued): tests/cpp/table_host.cpp holds it to its properties under a sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A null pointer or an empty range shares none.
inline bool akz_ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// the inputs of a call are const: true when no output lies over one of them
inline bool akz_outputs_clear_of_inputs(const void* const* in, const size_t* in_bytes, int n_in, const void* const* out, const size_t* out_bytes,
                                        int n_out)
{
    for (int i = 0; i < n_in; ++i)
        for (int o = 0; o < n_out; ++o)
            if (akz_ranges_overlap(in[i], in_bytes[i], out[o], out_bytes[o])) return false;
    return true;
}

// a host list of distinct blocks below n_blocks; seen [n_blocks] says which
inline bool akz_distinct_blocks(const uint32_t* blocks, uint32_t n, uint32_t n_blocks, std::vector<unsigned char>* seen)
{
    seen->assign(n_blocks, 0);
    for (uint32_t v = 0; v < n; ++v) {
        if (blocks[v] >= n_blocks || (*seen)[blocks[v]]) return false;
        (*seen)[blocks[v]] = 1;
    }
    return true;
}

// The regions of a call's scratch, one behind the other on 256-byte boundaries.  An entry point takes its regions in order,
// grows the scratch to size() and forms every pointer as base + offset; regions taken one after another are contiguous, so a
// run of them is filled with one memset whose length is the difference of two offsets.  (A take of no bytes takes no room:
// its offset is the next region's.  No stage has one — every size carries a + 1 or a count the entry point refuses at 0.)
struct AkzScratchPlan {
    size_t total = 0;
    size_t take(size_t bytes)
    {
        const size_t at = total;
        total += (bytes + 255) / 256 * 256;
        return at;
    }
    size_t size() const { return total; }
};
