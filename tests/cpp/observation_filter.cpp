// observation_filter.cpp — cv_sfm::ObservationFilter of include/akaze.hpp from a native process (no Python, no PyTorch) linked to
// libakz.so: one landmark table read from a file, device buffers from hipMalloc, one pass of the filter, every output printed.
// usage: observation_filter table.bin
// table.bin: u32 {n_blocks, cap, n_landmarks, n_obs, n_recons}, rs_camera, akz_keypoint [n_blocks][cap], f64 poses [n_blocks][12],
//            u32 obs_start [n_landmarks + 1], u32 obs [n_obs][2], u32 recon_start [n_recons + 1], u32 view_start [n_recons + 1]
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

template <class T>
static void show(const char* name, const std::vector<T>& v, size_t n)
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
    std::vector<rs_camera> cam(1);
    if (!take(fp, head) || !take(fp, cam)) return 2;
    const uint32_t n_blocks = head[0], cap = head[1], n_lm = head[2], n_obs = head[3], n_recons = head[4];
    std::vector<akz_keypoint> kps((size_t)n_blocks * cap);
    std::vector<double> poses(12 * (size_t)n_blocks);
    std::vector<uint32_t> start((size_t)n_lm + 1), obs(2 * (size_t)n_obs), recon_start((size_t)n_recons + 1), view_start((size_t)n_recons + 1);
    if (!take(fp, kps) || !take(fp, poses) || !take(fp, start) || !take(fp, obs) || !take(fp, recon_start) || !take(fp, view_start)) return 2;
    fclose(fp);

    // one buffer for everything the pass writes: keep, state, reason, robust (bytes), then the words
    const size_t room = n_obs ? n_obs : 1, lm_room = n_lm ? n_lm : 1;
    const size_t n_bytes = (room + 3 * lm_room + 3) / 4 * 4;
    const size_t n_words = (n_lm + 1) + 4 * room + 2 + n_recons * (1 + (size_t)RS_OF_STATS);
    void *d_kps, *d_poses, *d_start, *d_obs, *d_rs, *d_vs, *d_out;
    HIPOK(upload(kps, &d_kps));
    HIPOK(upload(poses, &d_poses));
    HIPOK(upload(start, &d_start));
    HIPOK(upload(obs, &d_obs));
    HIPOK(upload(recon_start, &d_rs));
    HIPOK(upload(view_start, &d_vs));
    HIPOK(hipMalloc(&d_out, n_bytes + 4 * n_words));
    HIPOK(hipMemset(d_out, 0xA5, n_bytes + 4 * n_words));
    unsigned char* b = static_cast<unsigned char*>(d_out);
    uint32_t* w = reinterpret_cast<uint32_t*>(b + n_bytes);
    uint32_t *d_start_out = w, *d_obs_out = w + n_lm + 1, *d_split_out = d_obs_out + 2 * room, *d_counts = d_split_out + 2 * room,
             *d_verdict = d_counts + 2, *d_stats = d_verdict + n_recons;
    try {
        cv_sfm::ObservationFilter filter;
        filter.filter_device(d_kps, cap, n_blocks, d_poses, cam[0], d_start, d_obs, n_obs, n_lm, d_rs, d_vs, n_recons, nullptr, b, b + room,
                             b + room + lm_room, b + room + 2 * lm_room, d_start_out, d_obs_out, d_split_out, d_counts, d_verdict, d_stats);
        filter.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::vector<unsigned char> ob(n_bytes);
    std::vector<uint32_t> ow(n_words);
    HIPOK(hipMemcpy(ob.data(), b, n_bytes, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(ow.data(), w, 4 * n_words, hipMemcpyDeviceToHost));
    const uint32_t* counts = ow.data() + (n_lm + 1) + 4 * room;
    show("keep", ob, n_obs);
    show("states", std::vector<unsigned char>(ob.begin() + room, ob.end()), n_lm);
    show("reasons", std::vector<unsigned char>(ob.begin() + room + lm_room, ob.end()), n_lm);
    show("robust", std::vector<unsigned char>(ob.begin() + room + 2 * lm_room, ob.end()), n_lm);
    show("start", ow, (size_t)n_lm + 1);
    show("obs", std::vector<uint32_t>(ow.begin() + n_lm + 1, ow.end()), 2 * (size_t)counts[0]);
    show("split", std::vector<uint32_t>(ow.begin() + n_lm + 1 + 2 * room, ow.end()), 2 * (size_t)counts[1]);
    show("counts", std::vector<uint32_t>(counts, counts + 2), 2);
    show("verdicts", std::vector<uint32_t>(counts + 2, counts + 2 + n_recons), n_recons);
    show("stats", std::vector<uint32_t>(counts + 2 + n_recons, counts + 2 + n_recons + n_recons * (size_t)RS_OF_STATS), n_recons * (size_t)RS_OF_STATS);
    for (void* p : {d_kps, d_poses, d_start, d_obs, d_rs, d_vs, d_out}) (void)hipFree(p);
    printf("observation_filter ok\n");
    return 0;
}
