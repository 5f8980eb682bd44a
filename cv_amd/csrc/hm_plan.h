// hm_plan.h — the recoding plan of one k-NN call of the matcher (hm_match.hip: launch_knn).  Host arithmetic only: nothing
// here touches the device, and the header includes nothing of HIP (tests/cpp/hm_plan.cpp compiles it alone).
//
// The MFMA kernels search +-1 recoded copies of the descriptor blocks (k_expand / k_expand4 write them into the context's
// d_exp).  The plan says which blocks a call's problems reference — one expand job each — and where in d_exp every
// problem finds its queries and its targets.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

struct HmPlanJob {
    const void* src;     // the descriptor block
    const void* count;   // its device count
    uint32_t cap;
    size_t off;          // word offset of the recoded block inside d_exp, cap * words_per_descriptor words long
};

struct HmPlan {
    std::vector<HmPlanJob> jobs;        // at most 2 per problem (what knn_stage_bytes reserves)
    std::vector<size_t> q_off, t_off;   // per problem: word offset of its recoded queries / targets (the `off` of their job)
    size_t words = 0;                   // of all jobs together
    uint32_t max_cap = 0;               // largest capacity of any block
};

// `Prob` carries q, nq, q_cap, t, nt, t_cap (HmProb of hm_match.hip).  words_per_descriptor: 64 (FP4) or 128 (int8).
template <typename Prob>
inline HmPlan hm_plan_recoding(const Prob* probs, uint32_t n_probs, size_t words_per_descriptor)
{
    HmPlan P;
    P.q_off.resize(n_probs);
    P.t_off.resize(n_probs);
    // block -> its jobs (a window call has thousands of problems over few blocks).  A job recodes rows [0, min(*count, cap)) of
    // its block, so one address met with another count or another capacity is another job: a buffer passed both as the
    // queries and as the targets of a call, each side with its own counts, must not share the shorter side's recoding.
    std::unordered_multimap<const void*, size_t> seen;
    auto recoded = [&](const void* src, const void* count, uint32_t cap) -> size_t {
        const auto same = seen.equal_range(src);
        for (auto it = same.first; it != same.second; ++it)
            if (P.jobs[it->second].count == count && P.jobs[it->second].cap == cap) return P.jobs[it->second].off;
        seen.emplace(src, P.jobs.size());
        P.jobs.push_back(HmPlanJob{src, count, cap, P.words});
        P.words += (size_t)cap * words_per_descriptor;
        if (cap > P.max_cap) P.max_cap = cap;
        return P.jobs.back().off;
    };
    for (uint32_t i = 0; i < n_probs; ++i) {
        P.q_off[i] = recoded(probs[i].q, probs[i].nq, probs[i].q_cap);
        P.t_off[i] = recoded(probs[i].t, probs[i].nt, probs[i].t_cap);
    }
    return P;
}
