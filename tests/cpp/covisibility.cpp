// covisibility.cpp — cv_sfm::ViewConstraints and cv_sfm::PoseGraph::rows of include/akaze.hpp from a native process (no Python,
// no PyTorch) linked to libakz.so: one landmark table read from a file, device buffers from hipMalloc, the candidates of every
// target and the rows of their triples, every output printed.
// usage: covisibility table.bin
// table.bin: u32 {n_blocks, cap, n_landmarks, n_obs, n_targets}, rs_covisibility_params, u32 obs_start [n_landmarks + 1],
//            u32 obs [n_obs][2], u8 reason [n_landmarks], u32 targets [n_targets]
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
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

template <class T>
static hipError_t upload(const std::vector<T>& src, void** d)
{
    const size_t bytes = sizeof(T) * (src.empty() ? 1 : src.size());
    hipError_t e = hipMalloc(d, bytes);
    if (e == hipSuccess && !src.empty()) e = hipMemcpy(*d, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice);
    return e;
}

static void show(const char* name, const uint32_t* v, size_t n)
{
    printf("%s", name);
    for (size_t i = 0; i < n; ++i) printf(" %u", (unsigned)v[i]);
    printf("\n");
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint32_t> head(5);
    std::vector<rs_covisibility_params> prm(1);
    if (!take(fp, head) || !take(fp, prm)) return 2;
    const uint32_t n_blocks = head[0], cap = head[1], n_lm = head[2], n_obs = head[3], n_targets = head[4];
    std::vector<uint32_t> start((size_t)n_lm + 1), obs(2 * (size_t)n_obs), targets(n_targets);
    std::vector<unsigned char> reason(n_lm);
    if (!take(fp, start) || !take(fp, obs) || !take(fp, reason) || !take(fp, targets)) return 2;
    fclose(fp);

    void *d_start, *d_obs, *d_reason, *d_targets, *d_out = nullptr;
    HIPOK(upload(start, &d_start));
    HIPOK(upload(obs, &d_obs));
    HIPOK(upload(reason, &d_reason));
    HIPOK(upload(targets, &d_targets));
    size_t n_slots = 0, n_lm_out = 0, n_words = 0;
    try {
        cv_sfm::PoseGraph graph;
        cv_sfm::ViewConstraints vc(graph.context());
        vc.params() = prm[0];
        n_slots = (size_t)n_targets * vc.limit();
        n_lm_out = n_slots * prm[0].optimization_maximum_landmarks;
        // views, lm_start, lm, slot_count, verdict, stats, row_start, row_edges, flags
        n_words = 3 * n_slots + (n_slots + 1) + 3 * n_lm_out + n_slots + n_targets * (1 + (size_t)RS_CV_STATS) + (n_blocks + 1) + 6 * n_slots + 1;
        HIPOK(hipMalloc(&d_out, 4 * n_words));
        HIPOK(hipMemset(d_out, 0xA5, 4 * n_words));
        uint32_t* w = static_cast<uint32_t*>(d_out);
        uint32_t *d_views = w, *d_lm_start = d_views + 3 * n_slots, *d_lm = d_lm_start + n_slots + 1, *d_count = d_lm + 3 * n_lm_out,
                 *d_verdict = d_count + n_slots, *d_stats = d_verdict + n_targets, *d_row_start = d_stats + n_targets * (size_t)RS_CV_STATS,
                 *d_row_edges = d_row_start + n_blocks + 1, *d_flags = d_row_edges + 6 * n_slots;
        vc.candidates_device(d_start, d_obs, n_obs, n_lm, cap, n_blocks, d_reason, d_targets, n_targets, d_views, d_lm_start, d_lm, d_count,
                             d_verdict, d_stats);
        graph.rows(d_views, (uint32_t)n_slots, n_blocks, d_row_start, d_row_edges, d_flags);
        graph.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::vector<uint32_t> ow(n_words);
    HIPOK(hipMemcpy(ow.data(), d_out, 4 * n_words, hipMemcpyDeviceToHost));
    const uint32_t* p = ow.data();
    show("views", p, 3 * n_slots);
    p += 3 * n_slots;
    show("lm_start", p, n_slots + 1);
    const size_t filled = p[n_slots];
    p += n_slots + 1;
    show("lm", p, 3 * filled);
    p += 3 * n_lm_out;
    show("counts", p, n_slots);
    p += n_slots;
    show("verdicts", p, n_targets);
    p += n_targets;
    show("stats", p, n_targets * (size_t)RS_CV_STATS);
    p += n_targets * (size_t)RS_CV_STATS;
    show("row_start", p, (size_t)n_blocks + 1);
    p += n_blocks + 1;
    show("row_edges", p, 6 * n_slots);
    p += 6 * n_slots;
    show("flags", p, 1);
    for (void* q : {d_start, d_obs, d_reason, d_targets, d_out}) (void)hipFree(q);
    printf("covisibility ok\n");
    return 0;
}
