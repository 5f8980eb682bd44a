// The host half of the observation-table stages (cv_amd/csrc/rs_table_host.h) on its own: the overlap rule against the plain
// statement of two intervals sharing a byte, the view-list check on its edge cases, the scratch plan's offsets.  Exits 1 on the
// first failed check (tests/test_table_host.py builds it with a plain C++ compiler and -fsanitize=address,undefined).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../cv_amd/csrc/rs_table_host.h"

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__);                 \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

static void check_overlap()
{
    const char* what = "akz_ranges_overlap";
    static unsigned char arena[8];
    long pairs = 0, hits = 0;
    // starts 0..4 and a null pointer, lengths 0..4: every range ends inside the arena
    for (int as = -1; as <= 4; ++as)
        for (int al = 0; al <= 4; ++al)
            for (int bs = -1; bs <= 4; ++bs)
                for (int bl = 0; bl <= 4; ++bl) {
                    const void* a = as < 0 ? nullptr : arena + as;
                    const void* b = bs < 0 ? nullptr : arena + bs;
                    bool share = false;                              // is there a byte of the arena in both?
                    if (as >= 0 && bs >= 0)
                        for (int k = 0; k < 8; ++k) share = share || (k >= as && k < as + al && k >= bs && k < bs + bl);
                    CHECK(akz_ranges_overlap(a, (size_t)al, b, (size_t)bl) == share);
                    CHECK(akz_ranges_overlap(b, (size_t)bl, a, (size_t)al) == share);
                    ++pairs;
                    hits += share;
                }
    CHECK(pairs == 6 * 5 * 6 * 5 && hits > 0 && hits < pairs);
    // the double loop: one output over one input refuses, whichever pair it is; null and empty entries never do
    const void* in[3] = {arena, nullptr, arena + 2};
    const size_t in_bytes[3] = {2, 4, 0};
    const void* out[2] = {arena + 2, arena + 6};
    const size_t out_bytes[2] = {4, 2};
    CHECK(akz_outputs_clear_of_inputs(in, in_bytes, 3, out, out_bytes, 2));
    CHECK(akz_outputs_clear_of_inputs(in, in_bytes, 0, out, out_bytes, 2) && akz_outputs_clear_of_inputs(in, in_bytes, 3, out, out_bytes, 0));
    for (int i = 0; i < 3; ++i)
        for (int o = 0; o < 2; ++o) {
            const void* in2[3] = {in[0], in[1], in[2]};
            size_t in2_bytes[3] = {in_bytes[0], in_bytes[1], in_bytes[2]};
            in2[i] = (const unsigned char*)out[o] + out_bytes[o] - 1;  // the output's last byte
            in2_bytes[i] = 1;
            CHECK(!akz_outputs_clear_of_inputs(in2, in2_bytes, 3, out, out_bytes, 2));
        }
    printf("overlap: %ld pairs, %ld share a byte\n", pairs, hits);
}

static void check_distinct()
{
    const char* what = "akz_distinct_blocks";
    std::vector<unsigned char> seen(3, 7);
    CHECK(akz_distinct_blocks(nullptr, 0, 5, &seen) && seen == std::vector<unsigned char>(5, 0));      // an empty list
    const uint32_t repeated[3] = {1, 3, 1}, at_end[2] = {0, 5}, last[3] = {4, 0, 2};
    CHECK(!akz_distinct_blocks(repeated, 3, 5, &seen));
    CHECK(akz_distinct_blocks(repeated, 2, 5, &seen) && seen == std::vector<unsigned char>({0, 1, 0, 1, 0}));
    CHECK(!akz_distinct_blocks(at_end, 2, 5, &seen));                                                   // a block equal to n_blocks
    CHECK(akz_distinct_blocks(last, 3, 5, &seen) && seen == std::vector<unsigned char>({1, 0, 1, 0, 1}));   // n_blocks - 1
    CHECK(!akz_distinct_blocks(last, 1, 4, &seen) && !akz_distinct_blocks(last, 1, 0, &seen) && seen.empty());
    printf("distinct blocks hold\n");
}

static void check_plan()
{
    const char* what = "AkzScratchPlan";
    const size_t bytes[8] = {32, 1, 255, 256, 257, 4 * 1025, 4, 1000003};
    AkzScratchPlan plan;
    CHECK(plan.size() == 0);
    size_t last = 0, last_len = 0;
    for (int k = 0; k < 8; ++k) {
        const size_t at = plan.take(bytes[k]);
        CHECK(at % 256 == 0 && (k == 0 ? at == 0 : at > last));      // multiples of 256, strictly ascending
        CHECK(k == 0 || at == last + last_len);                      // one behind the other: a run of regions is contiguous
        last = at;
        last_len = (bytes[k] + 255) / 256 * 256;
        CHECK(last_len >= bytes[k] && last_len < bytes[k] + 256);
        CHECK(plan.size() == last + last_len);                       // the last offset plus its aligned length
    }
    // no stage takes an empty region (every size carries a + 1 or a count refused at 0), so an empty take takes no room: its
    // offset is the next region's
    const size_t empty = plan.take(0), next = plan.take(4);
    CHECK(empty == last + last_len && next == empty && plan.size() == next + 256);
    printf("plan: %zu bytes\n", plan.size());
}

int main()
{
    check_overlap();
    check_distinct();
    check_plan();
    printf("the table stages' host half holds\n");
    return 0;
}
