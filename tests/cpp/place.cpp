// place.cpp — cv_sfm::FrameIndex of include/akaze.hpp from a native process (no Python, no PyTorch) linked to libakz.so: a frame
// table read from a file, device buffers from hipMalloc, the search for a batch of queries, the counts and verdicts printed.
// usage: place call.bin
// call.bin: u32 {n_stored, hash_bytes, nq, num_similar, num_recent, recent_threshold, search_num, has_visible},
//           u8 hashes [n_stored][hash_bytes], u32 feed / pos / recon / view [n_stored], u32 query [nq], u32 visible [nq] (if has_visible)
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
    std::vector<uint32_t> head(8);
    if (!take(fp, head)) return 2;
    const uint32_t n = head[0], hb = head[1], nq = head[2];
    std::vector<uint8_t> hashes((size_t)n * hb);
    std::vector<uint32_t> feed(n), pos(n), recon(n), view(n), query(nq), visible(head[7] ? nq : 0);
    if (!take(fp, hashes) || !take(fp, feed) || !take(fp, pos) || !take(fp, recon) || !take(fp, view) || !take(fp, query) || !take(fp, visible)) return 2;
    fclose(fp);

    hm_place_params p = cv_sfm::FrameIndex::params();
    p.num_similar = head[3];
    p.num_recent = head[4];
    p.recent_threshold = head[5];
    p.search_num = head[6];
    const uint32_t room = cv_sfm::FrameIndex::room(p);
    const size_t rows = n ? n : 1, words = (size_t)nq * (room + 1) + 1;
    void *d_hashes, *d_feed, *d_pos, *d_recon, *d_view, *d_query, *d_visible, *d_found, *d_views, *d_group_recon, *d_group_start, *d_free, *d_counts,
        *d_verdict;
    HIPOK(hipMalloc(&d_hashes, rows * hb));
    for (void** d : {&d_feed, &d_pos, &d_recon, &d_view}) HIPOK(hipMalloc(d, sizeof(uint32_t) * rows));
    for (void** d : {&d_query, &d_visible, &d_verdict}) HIPOK(hipMalloc(d, sizeof(uint32_t) * (nq + 1)));
    for (void** d : {&d_found, &d_views, &d_group_recon, &d_group_start, &d_free}) HIPOK(hipMalloc(d, sizeof(uint32_t) * words));
    HIPOK(hipMalloc(&d_counts, sizeof(uint32_t) * ((size_t)nq * HM_PL_COUNTS + 1)));
    try {
        space::Matcher m(64);
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
        index.find(d_query, visible.empty() ? nullptr : d_visible, nq, p, room, d_found, d_views, d_group_recon, d_group_start, d_free, nullptr,
                   d_counts, d_verdict);
        index.sync();
        std::vector<uint32_t> counts((size_t)nq * HM_PL_COUNTS), verdict(nq);
        HIPOK(hipMemcpy(counts.data(), d_counts, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(verdict.data(), d_verdict, sizeof(uint32_t) * nq, hipMemcpyDeviceToHost));
        for (uint32_t q = 0; q < nq; ++q)
            printf("query %u verdict %u counts %u %u %u %u %u\n", q, verdict[q], counts[5 * q], counts[5 * q + 1], counts[5 * q + 2], counts[5 * q + 3],
                   counts[5 * q + 4]);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (void* d : {d_hashes, d_feed, d_pos, d_recon, d_view, d_query, d_visible, d_found, d_views, d_group_recon, d_group_start, d_free, d_counts, d_verdict})
        (void)hipFree(d);
    printf("place ok\n");
    return 0;
}
