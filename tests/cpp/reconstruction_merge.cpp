// reconstruction_merge.cpp — cv_sfm::ReconstructionMerge of include/akaze.hpp from a native process (no Python, no PyTorch)
// linked to libakz.so: two landmark tables and a landmark map read from a file, device buffers from hipMalloc, the merged table,
// every output printed.
// usage: reconstruction_merge call.bin
// call.bin: u32 {n_blocks, cap, n_dst, n_dst_obs, n_src, n_src_obs, map_room, n_src_views, bridge_block, has_skip},
//           u32 dst_start [n_dst + 1], u32 dst_obs [n_dst_obs][2], u32 src_start [n_src + 1], u32 src_obs [n_src_obs][2],
//           u32 map [map_room][2], u32 map_count [1], u32 src_blocks [n_src_views], u32 skip [n_src_views], f64 src_pose [12],
//           f64 poses [n_blocks][12]
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
    std::vector<uint32_t> head(10);
    if (!take(fp, head)) return 2;
    const uint32_t n_blocks = head[0], cap = head[1], n_dst = head[2], n_dst_obs = head[3], n_src = head[4], n_src_obs = head[5],
                   map_room = head[6], n_views = head[7], bridge = head[8];
    const bool has_skip = head[9] != 0;
    std::vector<uint32_t> dst_start((size_t)n_dst + 1), dst_obs(2 * (size_t)n_dst_obs), src_start((size_t)n_src + 1), src_obs(2 * (size_t)n_src_obs),
        map(2 * (size_t)map_room), map_count(1), src_blocks(n_views), skip(n_views);
    std::vector<double> src_pose(12), poses(12 * (size_t)n_blocks);
    if (!take(fp, dst_start) || !take(fp, dst_obs) || !take(fp, src_start) || !take(fp, src_obs) || !take(fp, map) || !take(fp, map_count) ||
        !take(fp, src_blocks) || !take(fp, skip) || !take(fp, src_pose) || !take(fp, poses))
        return 2;
    fclose(fp);

    const uint64_t obs_room64 = (uint64_t)n_dst_obs + n_src_obs, lm_room64 = (uint64_t)n_dst + n_src;
    if (obs_room64 > 0xFFFFFFFFull || lm_room64 >= 0xFFFFFFFFull) return 2;
    const uint32_t obs_room = (uint32_t)obs_room64, lm_room = (uint32_t)lm_room64;
    void *d_dst_start, *d_dst_obs, *d_src_start, *d_src_obs, *d_map, *d_map_count, *d_skip, *d_src_pose, *d_poses, *d_out;
    HIPOK(upload(dst_start, &d_dst_start));
    HIPOK(upload(dst_obs, &d_dst_obs));
    HIPOK(upload(src_start, &d_src_start));
    HIPOK(upload(src_obs, &d_src_obs));
    HIPOK(upload(map, &d_map));
    HIPOK(upload(map_count, &d_map_count));
    HIPOK(upload(skip, &d_skip));
    HIPOK(upload(src_pose, &d_src_pose));
    HIPOK(upload(poses, &d_poses));
    // one buffer for every word the call writes
    const size_t lm_words = (size_t)n_blocks * cap;
    const size_t n_words = ((size_t)lm_room + 1) + 2 * ((size_t)obs_room + 1) + RS_IR_COUNTS + lm_words + ((size_t)lm_room + 1) + ((size_t)n_src + 1) + 1;
    HIPOK(hipMalloc(&d_out, 4 * n_words));
    HIPOK(hipMemset(d_out, 0xA5, 4 * n_words));
    uint32_t* w = static_cast<uint32_t*>(d_out);
    uint32_t *d_start_out = w, *d_obs_out = d_start_out + lm_room + 1, *d_counts_out = d_obs_out + 2 * ((size_t)obs_room + 1),
             *d_landmarks_out = d_counts_out + RS_IR_COUNTS, *d_obs_counts_out = d_landmarks_out + lm_words,
             *d_src_key_out = d_obs_counts_out + lm_room + 1, *d_call_verdict = d_src_key_out + n_src + 1;
    try {
        cv_sfm::ReconstructionMerge merge;
        merge.incorporate(d_dst_start, d_dst_obs, n_dst_obs, n_dst, d_src_start, d_src_obs, n_src_obs, n_src, d_map, d_map_count, map_room, cap,
                          n_blocks, src_blocks, bridge, d_src_pose, has_skip ? d_skip : nullptr, obs_room, lm_room, d_poses, d_start_out, d_obs_out,
                          d_counts_out, d_landmarks_out, d_obs_counts_out, d_src_key_out, d_call_verdict);
        merge.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::vector<uint32_t> ow(n_words);
    HIPOK(hipMemcpy(ow.data(), w, 4 * n_words, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(poses.data(), d_poses, sizeof(double) * poses.size(), hipMemcpyDeviceToHost));
    const uint32_t* h = ow.data();
    const uint32_t* counts_out = h + (d_counts_out - w);
    show("counts", counts_out, RS_IR_COUNTS);
    show("start", h, (size_t)counts_out[0] + 1);
    show("obs", h + (d_obs_out - w), 2 * (size_t)counts_out[1]);
    show("landmarks", h + (d_landmarks_out - w), lm_words);
    show("obs_counts", h + (d_obs_counts_out - w), counts_out[0]);
    show("src_key", h + (d_src_key_out - w), n_src);
    show("call", h + (d_call_verdict - w), 1);
    printf("poses");
    for (double v : poses) printf(" %.17g", v);
    printf("\n");
    for (void* p : {d_dst_start, d_dst_obs, d_src_start, d_src_obs, d_map, d_map_count, d_skip, d_src_pose, d_poses, d_out}) (void)hipFree(p);
    printf("reconstruction_merge ok\n");
    return 0;
}
