// three_view.cpp — cv_sfm::ThreeViewInit of include/akaze.hpp from a native process (no Python, no PyTorch) linked to
// libakz.so: one triple read from a file, device buffers from hipMalloc, verdict, poses and stats printed bit for bit.
// usage: three_view scene.bin
// scene.bin: u32 {cap, n, n_first, n_second, patience, filter_iterations}, f64 camera {fx, fy, cx, cy}, f64 poses [2][12],
//            akz_keypoint [3][cap] (blocks centre, first, second), u32 triples [cap][3], first_only [cap][2], second_only [cap][2]
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
static bool take(FILE* fp, T* dst, size_t n)
{
    return fread(dst, sizeof(T), n, fp) == n;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    uint32_t head[6];
    double camv[4], poses[24];
    if (!take(fp, head, 6) || !take(fp, camv, 4) || !take(fp, poses, 24)) return 2;
    const uint32_t cap = head[0];
    std::vector<akz_keypoint> kps(3 * (size_t)cap);
    std::vector<uint32_t> triples(3 * (size_t)cap), first_only(2 * (size_t)cap), second_only(2 * (size_t)cap);
    if (!take(fp, kps.data(), kps.size()) || !take(fp, triples.data(), triples.size()) || !take(fp, first_only.data(), first_only.size()) ||
        !take(fp, second_only.data(), second_only.size()))
        return 2;
    fclose(fp);

    akz_keypoint* d_kps = nullptr;
    uint32_t *d_lists = nullptr, *d_counts = nullptr, *d_out = nullptr;
    double *d_in = nullptr, *d_pose = nullptr;
    unsigned char* d_masks = nullptr;
    HIPOK(hipMalloc((void**)&d_kps, sizeof(akz_keypoint) * kps.size()));
    HIPOK(hipMalloc((void**)&d_lists, sizeof(uint32_t) * 7 * cap));
    HIPOK(hipMalloc((void**)&d_counts, sizeof(uint32_t) * 3));
    HIPOK(hipMalloc((void**)&d_out, sizeof(uint32_t) * (1 + RS_TV_STATS)));
    HIPOK(hipMalloc((void**)&d_in, sizeof(double) * 24));
    HIPOK(hipMalloc((void**)&d_pose, sizeof(double) * 24));
    HIPOK(hipMalloc((void**)&d_masks, 3 * (size_t)cap));
    HIPOK(hipMemcpy(d_kps, kps.data(), sizeof(akz_keypoint) * kps.size(), hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_lists, triples.data(), sizeof(uint32_t) * 3 * cap, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_lists + 3 * (size_t)cap, first_only.data(), sizeof(uint32_t) * 2 * cap, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_lists + 5 * (size_t)cap, second_only.data(), sizeof(uint32_t) * 2 * cap, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_counts, head + 1, sizeof(uint32_t) * 3, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(d_in, poses, sizeof(poses), hipMemcpyHostToDevice));
    HIPOK(hipMemset(d_pose, 0, sizeof(double) * 24));
    HIPOK(hipMemset(d_masks, 0, 3 * (size_t)cap));
    HIPOK(hipMemset(d_out, 0, sizeof(uint32_t) * (1 + RS_TV_STATS)));

    try {
        cv_sfm::ThreeViewInit tv(1);
        tv.params().three_view_patience = head[4];
        tv.params().three_view_filter_loop_iterations = head[5];
        rs_camera cam{};
        cam.fx = camv[0]; cam.fy = camv[1]; cam.cx = camv[2]; cam.cy = camv[3];
        tv.init_batch_device(d_kps, cap, 3, {0}, {1}, {2}, cam, d_in, d_in + 12, d_lists, d_counts, d_lists + 3 * (size_t)cap, d_counts + 1,
                             d_lists + 5 * (size_t)cap, d_counts + 2, d_pose, d_out, d_masks, d_masks + cap, d_masks + 2 * (size_t)cap, d_out + 1);
        tv.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    uint32_t out[1 + RS_TV_STATS];
    double pose[24];
    std::vector<unsigned char> masks(3 * (size_t)cap);
    HIPOK(hipMemcpy(out, d_out, sizeof(out), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(pose, d_pose, sizeof(pose), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(masks.data(), d_masks, masks.size(), hipMemcpyDeviceToHost));
    printf("verdict %u\n", out[0]);
    printf("poses");
    for (double v : pose) {
        unsigned long long u;
        memcpy(&u, &v, sizeof u);
        printf(" %016llx", u);
    }
    printf("\nstats");
    for (int k = 0; k < RS_TV_STATS; ++k) printf(" %u", out[1 + k]);
    uint32_t sums[3] = {0, 0, 0};
    for (int m = 0; m < 3; ++m)
        for (uint32_t i = 0; i < cap; ++i) sums[m] += masks[m * (size_t)cap + i];
    printf("\nmasks %u %u %u\n", sums[0], sums[1], sums[2]);
    hipFree(d_kps); hipFree(d_lists); hipFree(d_counts); hipFree(d_out); hipFree(d_in); hipFree(d_pose); hipFree(d_masks);
    printf("three_view ok\n");
    return 0;
}
