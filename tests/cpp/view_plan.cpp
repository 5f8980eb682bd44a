// view_plan.cpp — cv_sfm::FrameIndex::plan_views and the planned search of include/akaze.hpp from a native process (no Python, no
// PyTorch) linked to libakz.so: a frame table read from a file, the search for a batch of queries, the plan behind it on the
// matcher's stream with no wait in between, then the k = 3 search and the landmark choice over blocks of zero descriptors; the
// frames' verdicts and list lengths and the call's counts printed.
// usage: view_plan call.bin
// call.bin: u32 {n_stored, hash_bytes, nq, num_similar, num_recent, recent_threshold, search_num, has_visible, n_views, n_blocks,
//                exp_blocks, has_pick, by_recon, cap},
//           u8 hashes [n_stored][hash_bytes], u32 feed / pos / recon / view [n_stored], u32 query [nq], u32 visible [nq] (if has_visible),
//           u32 pick [nq] (if has_pick)
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include "akaze.hpp"

#define HIPOK(x)                                                                      \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) {                                                       \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
            return 4;                                                                 \
        }                                                                             \
    } while (0)

template <class T>
static bool take(FILE* fp, std::vector<T>& dst)
{
    return dst.empty() || fread(dst.data(), sizeof(T), dst.size(), fp) == dst.size();
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint32_t> head(14);
    if (!take(fp, head)) return 2;
    const uint32_t n = head[0], hb = head[1], nq = head[2], V = head[8], n_blocks = head[9], exp_blocks = head[10], cap = head[13];
    std::vector<uint8_t> hashes((size_t)n * hb);
    std::vector<uint32_t> feed(n), pos(n), recon(n), view(n), query(nq), visible(head[7] ? nq : 0), pick(head[11] ? nq : 0);
    if (!take(fp, hashes) || !take(fp, feed) || !take(fp, pos) || !take(fp, recon) || !take(fp, view) || !take(fp, query) || !take(fp, visible) ||
        !take(fp, pick))
        return 2;
    fclose(fp);
    if (nq == 0 || V == 0 || cap == 0 || n_blocks == 0) return 2;

    hm_place_params p = cv_sfm::FrameIndex::params();
    p.num_similar = head[3];
    p.num_recent = head[4];
    p.recent_threshold = head[5];
    p.search_num = head[6];
    const uint32_t room = cv_sfm::FrameIndex::room(p);
    const size_t rows = n ? n : 1, words = (size_t)nq * (room + 1) + 1;
    void *d_hashes, *d_feed, *d_pos, *d_recon, *d_view, *d_query, *d_visible, *d_found, *d_views, *d_group_recon, *d_group_start, *d_free, *d_counts,
        *d_verdict, *d_pick, *d_view_idx, *d_n_views, *d_plan_verdict, *d_plan_counts, *d_descs, *d_desc_counts, *d_landmarks, *d_knn, *d_best,
        *d_decision;
    HIPOK(hipMalloc(&d_hashes, rows * hb));
    for (void** d : {&d_feed, &d_pos, &d_recon, &d_view}) HIPOK(hipMalloc(d, sizeof(uint32_t) * rows));
    for (void** d : {&d_query, &d_visible, &d_verdict, &d_pick, &d_n_views, &d_plan_verdict}) HIPOK(hipMalloc(d, sizeof(uint32_t) * (nq + 1)));
    for (void** d : {&d_found, &d_views, &d_group_recon, &d_group_start, &d_free}) HIPOK(hipMalloc(d, sizeof(uint32_t) * words));
    HIPOK(hipMalloc(&d_counts, sizeof(uint32_t) * ((size_t)nq * HM_PL_COUNTS + 1)));
    HIPOK(hipMalloc(&d_view_idx, sizeof(uint32_t) * (size_t)nq * V));
    HIPOK(hipMalloc(&d_plan_counts, sizeof(uint32_t) * HM_VP_COUNTS));
    // the descriptor table: n_blocks stored blocks and the nq new frames' behind them, all of zero descriptors, one feature each
    const size_t blocks = (size_t)n_blocks + nq;
    HIPOK(hipMalloc(&d_descs, blocks * cap * 64));
    HIPOK(hipMemset(d_descs, 0, blocks * cap * 64));
    HIPOK(hipMalloc(&d_desc_counts, sizeof(uint32_t) * blocks));
    HIPOK(hipMalloc(&d_landmarks, sizeof(uint32_t) * blocks * cap));
    HIPOK(hipMemset(d_landmarks, 0, sizeof(uint32_t) * blocks * cap));
    HIPOK(hipMalloc(&d_knn, sizeof(akz_neighbor) * (size_t)nq * V * cap * 3));
    HIPOK(hipMalloc(&d_best, sizeof(uint32_t) * 2 * 3 * (size_t)nq * cap));
    HIPOK(hipMalloc(&d_decision, sizeof(uint32_t) * (size_t)nq * cap));
    try {
        space::Matcher m(cap);
        cv_sfm::FrameIndex index(m, d_hashes, d_feed, d_pos, d_recon, d_view, n, hb);
        const cv_sfm::FrameIndex::Rows tail = index.append_rows(n);
        HIPOK(hipMemcpy(tail.hashes, hashes.data(), hashes.size(), hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(tail.feed, feed.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(tail.pos, pos.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        const cv_sfm::FrameIndex::Rows stored = index.set_views(0, n);
        HIPOK(hipMemcpy(stored.recon, recon.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(stored.view, view.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(d_query, query.data(), sizeof(uint32_t) * nq, hipMemcpyHostToDevice));
        if (!visible.empty()) HIPOK(hipMemcpy(d_visible, visible.data(), sizeof(uint32_t) * nq, hipMemcpyHostToDevice));
        if (!pick.empty()) HIPOK(hipMemcpy(d_pick, pick.data(), sizeof(uint32_t) * nq, hipMemcpyHostToDevice));
        const std::vector<uint32_t> ones(blocks, 1u);
        HIPOK(hipMemcpy(d_desc_counts, ones.data(), sizeof(uint32_t) * blocks, hipMemcpyHostToDevice));
        std::vector<uint32_t> iq(nq);
        for (uint32_t f = 0; f < nq; ++f) iq[f] = n_blocks + f;

        const cv_sfm::FrameIndex::ViewPlan plan{d_view_idx, d_n_views, d_plan_verdict, d_plan_counts, nq, V, n_blocks, exp_blocks};
        index.find(d_query, visible.empty() ? nullptr : d_visible, nq, p, room, d_found, d_views, d_group_recon, d_group_start, d_free, nullptr,
                   d_counts, d_verdict);
        index.plan_views(d_views, d_group_recon, d_group_start, d_counts, d_verdict, room, pick.empty() ? nullptr : d_pick, head[12] != 0, plan);
        index.knn_planned(d_descs, d_desc_counts, cap, iq.data(), plan, 3, d_knn);
        index.best_of_views_planned(d_knn, d_desc_counts, cap, iq.data(), plan, 3, d_landmarks, 24, d_best, d_decision);
        index.sync();
        std::vector<uint32_t> counts(HM_VP_COUNTS), verdict(nq), lengths(nq);
        HIPOK(hipMemcpy(counts.data(), d_plan_counts, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(verdict.data(), d_plan_verdict, sizeof(uint32_t) * nq, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(lengths.data(), d_n_views, sizeof(uint32_t) * nq, hipMemcpyDeviceToHost));
        for (uint32_t f = 0; f < nq; ++f) printf("frame %u verdict %u views %u\n", f, verdict[f], lengths[f]);
        printf("counts %u %u %u %u\n", counts[0], counts[1], counts[2], counts[3]);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (void* d : {d_hashes, d_feed, d_pos, d_recon, d_view, d_query, d_visible, d_found, d_views, d_group_recon, d_group_start, d_free, d_counts,
                    d_verdict, d_pick, d_view_idx, d_n_views, d_plan_verdict, d_plan_counts, d_descs, d_desc_counts, d_landmarks, d_knn, d_best, d_decision})
        (void)hipFree(d);
    printf("view_plan ok\n");
    return 0;
}
