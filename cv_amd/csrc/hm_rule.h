// hm_rule.h — the reverse side of a symmetric match, asked as ONE question of the forward lists (hm_match.hip: k_decide,
// k_verify, k_pairs and the dispatcher; tests/cpp/hm_rule.cpp compiles this header alone).  Nothing of HIP in here.
//
// A forward-accepted pair (a, b = nn1(a), d0 = d(a, b)) survives the reverse check of symmetric_matching when a is b's nearest
// and b's list passes the accept rule: r0.index == a and accept(r0.distance, r1.distance).  With r0 = (d0, a) that is a
// statement about the OTHER queries only:
//   STRICT     d0 + pu <  r1.distance   <=>   no a' != a has d(a', b) <= d0 + pu
//   BETTER_BY  d0 + pu <= r1.distance   <=>   no a' != a has d(a', b) <= d0 + pu - 1          (pu >= 1)
// and whenever the bound tau is >= d0 the absence of such a rival also makes a the nearest (every other distance is larger,
// so no tie is decided by index).  BETTER_BY with pu = 0 has tau = d0 - 1: ties at d0 go to the lower index, which the bound
// cannot say; LOWE compares floats.  Both keep the reverse search.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HM_RULE_HD __host__ __device__
#else
#define HM_RULE_HD
#endif

constexpr int kHmRuleStrict = 0, kHmRuleBetterBy = 1;   // HM_RULE_BETTER_BY_STRICT, HM_RULE_BETTER_BY of include/akz.h
constexpr uint32_t kHmMaxDistance = 512;               // of two 64-byte rows
// parameters from here on could wrap d0 + pu in 32 bits; that arithmetic is accept()'s, so they keep the reverse search
constexpr uint32_t kHmRuleMaxParam = 1u << 30;

// Does the rival bound stand in for the reverse search under (rule, pu)?
HM_RULE_HD constexpr bool hm_rival_bound_applies(int rule, uint32_t pu)
{
    return pu < kHmRuleMaxParam && (rule == kHmRuleStrict || (rule == kHmRuleBetterBy && pu >= 1u));
}

// tau of the pair whose forward distance is d0: the pair survives iff no other query lies within tau of its target.
// -1: not applicable.  Otherwise d0 <= tau <= 512 (a bound past the largest distance says no more than 512 does; d0 itself
// is at most 512 for a neighbour that exists).
HM_RULE_HD constexpr int32_t hm_rival_bound(int rule, uint32_t pu, uint32_t d0)
{
    if (!hm_rival_bound_applies(rule, pu) || d0 > kHmMaxDistance) return -1;
    const uint32_t t = d0 + pu - (rule == kHmRuleBetterBy ? 1u : 0u);
    return (int32_t)(t < kHmMaxDistance ? t : kHmMaxDistance);
}
