// pose_graph.cpp — cv_sfm::PoseGraph of include/akaze.hpp from a native process (no Python, no PyTorch) linked to libakz.so:
// one batch read from a file, rows from PoseGraph::flatten, device buffers from hipMalloc, verdicts, view states, stats and
// poses printed bit for bit.
// usage: pose_graph batch.bin
// batch.bin: u32 {n_views, n_graphs, n_constraints, iterations}, f64 poses [n_views][12], u32 graph_start [n_graphs + 1],
//            u32 views [n][3], u32 constraint verdicts [n], f64 constraint poses [n][24]
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

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint32_t> head(4);
    if (!take(fp, head)) return 2;
    const uint32_t n_views = head[0], n_graphs = head[1], n = head[2];
    std::vector<double> poses(12 * (size_t)n_views), cposes(24 * (size_t)n);
    std::vector<uint32_t> graph_start((size_t)n_graphs + 1), views(3 * (size_t)n), cverdict(n), row_start, row_edges;
    if (!take(fp, poses) || !take(fp, graph_start) || !take(fp, views) || !take(fp, cverdict) || !take(fp, cposes)) return 2;
    fclose(fp);
    if (!cv_sfm::PoseGraph::flatten(views, n_views, row_start, row_edges)) return 2;

    const size_t n_out = (size_t)n_graphs * (1 + RS_PG_STATS) + n_views;
    void *d_poses, *d_gs, *d_rs, *d_re, *d_views, *d_cverdict, *d_cposes, *d_edges, *d_out;
    HIPOK(upload(poses, &d_poses));
    HIPOK(upload(graph_start, &d_gs));
    HIPOK(upload(row_start, &d_rs));
    HIPOK(upload(row_edges, &d_re));
    HIPOK(upload(views, &d_views));
    HIPOK(upload(cverdict, &d_cverdict));
    HIPOK(upload(cposes, &d_cposes));
    HIPOK(hipMalloc(&d_edges, sizeof(double) * 72 * (n ? n : 1)));
    HIPOK(hipMalloc(&d_out, sizeof(uint32_t) * n_out));
    HIPOK(hipMemset(d_out, 0xA5, sizeof(uint32_t) * n_out));

    uint32_t* d_verdict = static_cast<uint32_t*>(d_out);
    try {
        cv_sfm::PoseGraph pg;
        pg.params().optimization_iterations = head[3];
        pg.edges_device(d_views, d_cposes, d_cverdict, n, d_edges);
        pg.relax_batch_device(d_poses, n_views, d_gs, n_graphs, d_rs, d_re, (uint32_t)row_edges.size(), d_views, d_cverdict, d_edges, n,
                              d_verdict, d_verdict + (size_t)n_graphs * (1 + RS_PG_STATS), d_verdict + n_graphs);
        pg.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::vector<uint32_t> out(n_out);
    HIPOK(hipMemcpy(out.data(), d_out, sizeof(uint32_t) * n_out, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(poses.data(), d_poses, sizeof(double) * poses.size(), hipMemcpyDeviceToHost));
    printf("verdicts");
    for (uint32_t g = 0; g < n_graphs; ++g) printf(" %u", out[g]);
    printf("\nstats");
    for (size_t k = 0; k < (size_t)RS_PG_STATS * n_graphs; ++k) printf(" %u", out[n_graphs + k]);
    printf("\nstates");
    for (uint32_t v = 0; v < n_views; ++v) printf(" %u", out[(size_t)n_graphs * (1 + RS_PG_STATS) + v]);
    printf("\nrows");
    for (uint32_t e : row_edges) printf(" %u", e);
    printf("\nposes");
    for (double v : poses) {
        unsigned long long u;
        memcpy(&u, &v, sizeof u);
        printf(" %016llx", u);
    }
    printf("\n");
    hipFree(d_poses); hipFree(d_gs); hipFree(d_rs); hipFree(d_re); hipFree(d_views); hipFree(d_cverdict); hipFree(d_cposes);
    hipFree(d_edges); hipFree(d_out);
    printf("pose_graph ok\n");
    return 0;
}
