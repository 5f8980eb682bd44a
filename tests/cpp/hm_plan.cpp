// The matcher's recoding plan (cv_amd/csrc/hm_plan.h) on the host alone: which descriptor blocks a k-NN call recodes and
// where every problem finds them.  Prints one line per case and exits 1 on the first failed check
// (tests/test_matcher_plan.py).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../cv_amd/csrc/hm_plan.h"

struct Prob {   // the fields of hm_match.hip's HmProb that the plan reads
    const void* q;
    const void* nq;
    uint32_t q_cap;
    const void* t;
    const void* nt;
    uint32_t t_cap;
};

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            printf("FAILED %s: %s (line %d)\n", what, #cond, __LINE__);                 \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

// what every plan promises, whatever the problems
static void check_plan(const char* what, const std::vector<Prob>& probs, size_t words, const HmPlan& P, size_t want_jobs)
{
    const size_t n = probs.size();
    CHECK(P.jobs.size() == want_jobs);
    CHECK(P.jobs.size() <= 2 * n);                                       // what knn_stage_bytes reserves
    CHECK(P.q_off.size() == n && P.t_off.size() == n);
    // the jobs' ranges [off, off + cap * words) are pairwise disjoint and sum to the total
    std::vector<std::pair<size_t, size_t>> ranges;
    size_t sum = 0;
    uint32_t max_cap = 0;
    for (const HmPlanJob& j : P.jobs) {
        ranges.emplace_back(j.off, j.off + (size_t)j.cap * words);
        sum += (size_t)j.cap * words;
        max_cap = std::max(max_cap, j.cap);
    }
    std::sort(ranges.begin(), ranges.end());
    for (size_t i = 0; i + 1 < ranges.size(); ++i) CHECK(ranges[i].second <= ranges[i + 1].first);
    for (const auto& r : ranges) CHECK(r.second <= P.words);
    CHECK(sum == P.words);
    CHECK(max_cap == P.max_cap);
    // no two jobs for one (address, count, capacity)
    for (size_t a = 0; a < P.jobs.size(); ++a)
        for (size_t b = a + 1; b < P.jobs.size(); ++b)
            CHECK(!(P.jobs[a].src == P.jobs[b].src && P.jobs[a].count == P.jobs[b].count && P.jobs[a].cap == P.jobs[b].cap));
    // every problem's offsets are those of the job of its own (address, count, capacity)
    auto job_of = [&](const void* src, const void* count, uint32_t cap) -> const HmPlanJob* {
        for (const HmPlanJob& j : P.jobs)
            if (j.src == src && j.count == count && j.cap == cap) return &j;
        return nullptr;
    };
    for (size_t i = 0; i < n; ++i) {
        const HmPlanJob* jq = job_of(probs[i].q, probs[i].nq, probs[i].q_cap);
        const HmPlanJob* jt = job_of(probs[i].t, probs[i].nt, probs[i].t_cap);
        CHECK(jq && jt);
        CHECK(P.q_off[i] == jq->off && P.t_off[i] == jt->off);
    }
    printf("ok %s: %zu problems, %zu jobs, %zu words\n", what, n, P.jobs.size(), P.words);
}

static void run(const char* what, const std::vector<Prob>& probs, size_t want_jobs)
{
    for (size_t words : {(size_t)64, (size_t)128})   // FP4, int8
        check_plan(what, probs, words, hm_plan_recoding(probs.data(), (uint32_t)probs.size(), words), want_jobs);
}

int main()
{
    // stand-ins for device memory: the plan compares addresses and never reads through them
    static unsigned char blocks[96][64];
    static uint32_t counts[96 + 2];
    const uint32_t cap = 70;

    run("no problems", {}, 0);
    {
        const HmPlan P = hm_plan_recoding((const Prob*)nullptr, 0, 64);
        const char* what = "no problems";
        CHECK(P.words == 0 && P.max_cap == 0 && P.jobs.empty() && P.q_off.empty() && P.t_off.empty());
    }
    for (uint32_t n : {1u, 2u, 7u, 1000u})
        run("n problems over one block pair", std::vector<Prob>(n, Prob{blocks[0], &counts[0], cap, blocks[1], &counts[1], 33}), 2);
    // one buffer as the queries and as the targets (test_one_buffer_as_queries_and_as_targets_with_different_counts)
    run("one buffer, same count and capacity", {Prob{blocks[0], &counts[0], cap, blocks[0], &counts[0], cap}}, 1);
    run("one buffer, another count", {Prob{blocks[0], &counts[0], cap, blocks[0], &counts[1], cap}}, 2);
    run("one buffer, another capacity", {Prob{blocks[0], &counts[0], cap, blocks[0], &counts[0], cap + 1}}, 2);
    run("one buffer, another count and capacity", {Prob{blocks[0], &counts[0], cap, blocks[0], &counts[1], 1}}, 2);
    {
        // blocks of one buffer under two count arrays, as hm_knn_batch_device builds them with d_q == d_t, d_nq != d_nt
        std::vector<Prob> probs;
        const uint32_t iq[] = {0, 1, 2, 0, 2}, it[] = {1, 0, 2, 2, 0};
        for (int p = 0; p < 5; ++p) probs.push_back(Prob{blocks[iq[p]], &counts[iq[p]], cap, blocks[it[p]], &counts[48 + it[p]], cap});
        run("three blocks under two count arrays", probs, 6);
    }
    run("symmetric pairs", {Prob{blocks[0], &counts[0], cap, blocks[1], &counts[1], cap},
                            Prob{blocks[1], &counts[1], cap, blocks[0], &counts[0], cap}}, 2);
    {
        // hm_match_batch_device, symmetric: three pairs over three blocks, forward problems then the reverse ones
        std::vector<Prob> probs(6);
        for (uint32_t p = 0; p < 3; ++p) {
            const uint32_t a = p, b = (p + 1) % 3;
            probs[p] = Prob{blocks[a], &counts[a], cap, blocks[b], &counts[b], cap};
            probs[3 + p] = Prob{blocks[b], &counts[b], cap, blocks[a], &counts[a], cap};
        }
        run("three symmetric pairs over three blocks", probs, 3);
    }
    {
        // a window call: 64 frames (blocks 32 .. 95) against their 32 predecessors each
        std::vector<Prob> probs;
        for (uint32_t f = 0; f < 64; ++f)
            for (uint32_t v = 0; v < 32; ++v) {
                const uint32_t a = 32 + f, b = a - 1 - v;
                probs.push_back(Prob{blocks[a], &counts[a], 8192, blocks[b], &counts[b], 8192});
            }
        run("window of 64 x 32 problems over 96 blocks", probs, 96);
    }
    {
        // capacities that differ: offsets follow each job's own length
        std::vector<Prob> probs;
        for (uint32_t p = 0; p < 9; ++p) probs.push_back(Prob{blocks[p], &counts[p], 1 + 37 * p, blocks[95 - p % 2], &counts[95], 513});
        run("mixed capacities", probs, 9 + 2);
    }
    printf("all plans hold\n");
    return 0;
}
