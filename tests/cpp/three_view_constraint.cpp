// three_view_constraint.cpp — cv_sfm::ThreeViewConstraints of include/akaze.hpp from a native process (no Python, no PyTorch)
// linked to libakz.so: one batch read from a file, device buffers from hipMalloc, verdicts, poses and stats printed bit for bit.
// usage: three_view_constraint batch.bin
// batch.bin: u32 {cap, n_blocks, n_constraints, n_lm, patience, maximum_landmarks}, f64 camera {fx, fy, cx, cy},
//            f64 poses [n_blocks][12], akz_keypoint [n_blocks][cap], u32 views [n][3], lm_start [n + 1], lm [n_lm][3]
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
    std::vector<uint32_t> head(6);
    std::vector<double> camv(4);
    if (!take(fp, head) || !take(fp, camv)) return 2;
    const uint32_t cap = head[0], n_blocks = head[1], n = head[2], n_lm = head[3];
    std::vector<double> poses(12 * (size_t)n_blocks);
    std::vector<akz_keypoint> kps((size_t)n_blocks * cap);
    std::vector<uint32_t> views(3 * (size_t)n), lm_start((size_t)n + 1), lm(3 * (size_t)n_lm);
    if (!take(fp, poses) || !take(fp, kps) || !take(fp, views) || !take(fp, lm_start) || !take(fp, lm)) return 2;
    fclose(fp);

    void *d_kps, *d_poses, *d_views, *d_start, *d_lm, *d_pose, *d_out;
    HIPOK(upload(kps, &d_kps));
    HIPOK(upload(poses, &d_poses));
    HIPOK(upload(views, &d_views));
    HIPOK(upload(lm_start, &d_start));
    HIPOK(upload(lm, &d_lm));
    HIPOK(hipMalloc(&d_pose, sizeof(double) * 24 * n));
    HIPOK(hipMalloc(&d_out, sizeof(uint32_t) * (1 + RS_TVC_STATS) * n));
    HIPOK(hipMemset(d_pose, 0, sizeof(double) * 24 * n));
    HIPOK(hipMemset(d_out, 0, sizeof(uint32_t) * (1 + RS_TVC_STATS) * n));

    try {
        cv_sfm::ThreeViewConstraints tvc;
        tvc.params().constraint_patience = head[4];
        tvc.params().optimization_maximum_landmarks = head[5];
        rs_camera cam{};
        cam.fx = camv[0]; cam.fy = camv[1]; cam.cx = camv[2]; cam.cy = camv[3];
        tvc.batch_device(d_kps, cap, n_blocks, d_poses, cam, d_views, d_start, d_lm, n_lm, n, d_pose, d_out,
                         static_cast<uint32_t*>(d_out) + n);
        tvc.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::vector<uint32_t> out((1 + RS_TVC_STATS) * (size_t)n);
    std::vector<double> pose(24 * (size_t)n);
    HIPOK(hipMemcpy(out.data(), d_out, sizeof(uint32_t) * out.size(), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(pose.data(), d_pose, sizeof(double) * pose.size(), hipMemcpyDeviceToHost));
    printf("verdicts");
    for (uint32_t s = 0; s < n; ++s) printf(" %u", out[s]);
    printf("\nposes");
    for (double v : pose) {
        unsigned long long u;
        memcpy(&u, &v, sizeof u);
        printf(" %016llx", u);
    }
    printf("\nstats");
    for (size_t k = 0; k < (size_t)RS_TVC_STATS * n; ++k) printf(" %u", out[n + k]);
    printf("\n");
    hipFree(d_kps); hipFree(d_poses); hipFree(d_views); hipFree(d_start); hipFree(d_lm); hipFree(d_pose); hipFree(d_out);
    printf("three_view_constraint ok\n");
    return 0;
}
