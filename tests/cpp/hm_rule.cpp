// The rival bound of a symmetric match (cv_amd/csrc/hm_rule.h) on the host alone: for every rule, parameter and forward
// distance the bound says exactly what the reverse check of symmetric_matching says about the nearest OTHER query of the
// pair's target.  No HIP, no library: g++ -std=c++17 tests/cpp/hm_rule.cpp.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../cv_amd/csrc/hm_rule.h"

// the accept rules as hm_match.hip's accept() and the reference's call sites state them (32-bit arithmetic)
static bool accept(int rule, uint32_t d0, uint32_t d1, uint32_t pu)
{
    return rule == kHmRuleStrict ? d0 + pu < d1 : d0 + pu <= d1;
}

// The reverse check for the pair (a, b) with d(a, b) = d0, when the nearest other query of b lies at distance `other` and
// has the higher or the lower index of the two: r0, r1 are b's two nearest in (distance, index) order, a tie to the lower index.
static bool reverse_keeps(int rule, uint32_t pu, uint32_t d0, uint32_t other, bool a_lower)
{
    const bool a_first = d0 < other || (d0 == other && a_lower);
    const uint32_t r0 = a_first ? d0 : other, r1 = a_first ? other : d0;
    return a_first && accept(rule, r0, r1, pu);
}

static_assert(hm_rival_bound(kHmRuleStrict, 24, 3) == 27, "STRICT: d0 + pu");
static_assert(hm_rival_bound(kHmRuleBetterBy, 24, 3) == 26, "BETTER_BY: d0 + pu - 1");
static_assert(hm_rival_bound(kHmRuleBetterBy, 1, 3) == 3, "BETTER_BY 1: tau = d0");
static_assert(hm_rival_bound(kHmRuleBetterBy, 0, 3) == -1, "BETTER_BY 0 keeps the search");
static_assert(hm_rival_bound(2, 24, 3) == -1, "LOWE keeps the search");
static_assert(hm_rival_bound(kHmRuleStrict, 0, 0) == 0 && hm_rival_bound(kHmRuleStrict, 600, 7) == 512, "ends of the range");
static_assert(!hm_rival_bound_applies(kHmRuleStrict, 0xFFFFFFF0u), "a parameter that wraps d0 + pu keeps the search");

int main()
{
    int failed = 0;
    long checked = 0;
    const uint32_t params[] = {0, 1, 2, 23, 24, 25, 100, 487, 511, 512, 513, 1000, 1u << 20, (1u << 30) - 1u};
    for (int rule = 0; rule <= 1; ++rule)
        for (uint32_t pu : params) {
            const bool applies = hm_rival_bound_applies(rule, pu);
            if (applies != (rule == kHmRuleStrict || pu >= 1)) {
                std::printf("FAILED applies(rule %d, pu %u) = %d\n", rule, pu, (int)applies);
                ++failed;
            }
            for (uint32_t d0 = 0; d0 <= 512; ++d0) {
                const int32_t tau = hm_rival_bound(rule, pu, d0);
                if (!applies) {
                    if (tau != -1) { std::printf("FAILED rule %d pu %u d0 %u: tau %d where nothing applies\n", rule, pu, d0, tau); ++failed; }
                    continue;
                }
                if (tau < (int32_t)d0 || tau > 512) { std::printf("FAILED rule %d pu %u d0 %u: tau %d out of [d0, 512]\n", rule, pu, d0, tau); ++failed; continue; }
                for (uint32_t other = 0; other <= 512; ++other, ++checked)
                    if (reverse_keeps(rule, pu, d0, other, false) != (other > (uint32_t)tau) ||
                        reverse_keeps(rule, pu, d0, other, true) != (other > (uint32_t)tau)) {
                        std::printf("FAILED rule %d pu %u d0 %u other %u: tau %d\n", rule, pu, d0, other, tau);
                        ++failed;
                    }
            }
            if (hm_rival_bound(rule, pu, 513) != -1 || hm_rival_bound(rule, pu, 1023) != -1) {
                std::printf("FAILED rule %d pu %u: a distance past 512 has a bound\n", rule, pu);
                ++failed;
            }
        }
    for (uint32_t pu : {1u << 30, 0x80000000u, 0xFFFFFFFFu})
        for (int rule = 0; rule <= 2; ++rule)
            if (hm_rival_bound_applies(rule, pu) || hm_rival_bound(rule, pu, 5) != -1) { std::printf("FAILED rule %d pu %u applies\n", rule, pu); ++failed; }
    std::printf("checked %ld (rule, pu, d0, other) cases\n", checked);
    if (failed) return 1;
    std::printf("all bounds hold\n");
    return 0;
}
