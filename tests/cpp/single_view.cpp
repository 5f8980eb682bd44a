// single_view.cpp — cv_sfm::SingleViewRefiner of include/akaze.hpp from a native process (no Python, no PyTorch) linked to
// libakz.so: one batch read from a file, device buffers from hipMalloc, one call, every output printed.
// usage: single_view batch.bin
// batch.bin: u32 {n_blocks, cap, n_landmarks, n_obs, n_world, n_rows, n_scenes, has_best, patience, loops}, f64 rate, rs_camera,
//            akz_keypoint [n_blocks][cap], f64 poses [n_blocks][12], u32 obs_start [n_landmarks + 1], u32 obs [n_obs][2],
//            f64 world [n_rows][4], u32 ik [n_scenes], u32 matches [n_scenes][cap][2], u32 nmatches [n_scenes],
//            u32 best [n_scenes][cap][3][2] (with has_best), f64 pose [n_scenes][12], u32 best_id [n_scenes],
//            u32 inliers [n_scenes][cap], u32 n_inliers [n_scenes]
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
    std::vector<uint32_t> head(10);
    std::vector<double> rate(1);
    std::vector<rs_camera> cam(1);
    if (!take(fp, head) || !take(fp, rate) || !take(fp, cam)) return 2;
    const uint32_t n_blocks = head[0], cap = head[1], n_lm = head[2], n_obs = head[3], n_world = head[4], n_rows = head[5], S = head[6];
    const bool has_best = head[7] != 0;
    std::vector<akz_keypoint> kps((size_t)n_blocks * cap);
    std::vector<double> poses(12 * (size_t)n_blocks), world(4 * (size_t)n_rows), pose(12 * (size_t)S);
    std::vector<uint32_t> start((size_t)n_lm + 1), obs(2 * (size_t)n_obs), ik(S), matches(2 * (size_t)S * cap), nmatches(S),
        best(has_best ? 6 * (size_t)S * cap : 0), best_id(S), inliers((size_t)S * cap), n_inliers(S);
    if (!take(fp, kps) || !take(fp, poses) || !take(fp, start) || !take(fp, obs) || !take(fp, world) || !take(fp, ik) || !take(fp, matches) ||
        !take(fp, nmatches) || !take(fp, best) || !take(fp, pose) || !take(fp, best_id) || !take(fp, inliers) || !take(fp, n_inliers))
        return 2;
    fclose(fp);

    void *d_kps, *d_poses, *d_start, *d_obs, *d_world, *d_matches, *d_nmatches, *d_best, *d_pose, *d_best_id, *d_inliers, *d_n_inliers, *d_out;
    HIPOK(upload(kps, &d_kps));
    HIPOK(upload(poses, &d_poses));
    HIPOK(upload(start, &d_start));
    HIPOK(upload(obs, &d_obs));
    HIPOK(upload(world, &d_world));
    HIPOK(upload(matches, &d_matches));
    HIPOK(upload(nmatches, &d_nmatches));
    HIPOK(upload(best, &d_best));
    HIPOK(upload(pose, &d_pose));
    HIPOK(upload(best_id, &d_best_id));
    HIPOK(upload(inliers, &d_inliers));
    HIPOK(upload(n_inliers, &d_n_inliers));
    // one buffer for everything the call writes: poses (f64), then the words, then the bytes
    const size_t n_words = (size_t)S * (2 + RS_SV_STATS), n_bytes = (size_t)S * cap;
    HIPOK(hipMalloc(&d_out, 96 * (size_t)S + 4 * n_words + n_bytes));
    HIPOK(hipMemset(d_out, 0xA5, 96 * (size_t)S + 4 * n_words + n_bytes));
    double* d_pose_out = static_cast<double*>(d_out);
    uint32_t* w = reinterpret_cast<uint32_t*>(d_pose_out + 12 * (size_t)S);
    uint32_t *d_verdict = w, *d_n_final = w + S, *d_stats = w + 2 * (size_t)S;
    unsigned char* d_final = reinterpret_cast<unsigned char*>(w + n_words);
    rs_ctx* ctx = nullptr;
    if (rs_create(0, 64, 64, &ctx) != AKZ_OK || rs_batch_reserve(ctx, S ? S : 1) != AKZ_OK) {
        fprintf(stderr, "no context\n");
        return 3;
    }
    try {
        cv_sfm::SingleViewRefiner refiner(ctx);
        refiner.params().single_view_patience = head[8];
        refiner.params().single_view_filter_loop_iterations = head[9];
        refiner.params().single_view_optimization_rate = rate[0];
        refiner.refine_batch_device(d_kps, cap, n_blocks, d_poses, cam[0], d_start, n_obs ? d_obs : nullptr, n_obs, n_lm, d_world, n_world, ik,
                                    d_matches, d_nmatches, has_best ? d_best : nullptr, d_pose, d_best_id, d_inliers, d_n_inliers, d_pose_out,
                                    d_verdict, d_final, d_n_final, d_stats);
        refiner.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::vector<double> op(12 * (size_t)S);
    std::vector<uint32_t> ow(n_words);
    std::vector<unsigned char> ob(n_bytes);
    HIPOK(hipMemcpy(op.data(), d_pose_out, 96 * (size_t)S, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(ow.data(), w, 4 * n_words, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(ob.data(), d_final, n_bytes, hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < S; ++s) {
        printf("scene %u %u %u", s, ow[s], ow[S + s]);
        for (int k = 0; k < RS_SV_STATS; ++k) printf(" %u", ow[2 * (size_t)S + (size_t)s * RS_SV_STATS + k]);
        printf("\npose");
        for (int k = 0; k < 12; ++k) {
            unsigned long long u;
            memcpy(&u, &op[12 * (size_t)s + k], 8);
            printf(" %llx", u);
        }
        printf("\nfinal");
        for (uint32_t i = 0; i < nmatches[s] && i < cap; ++i) printf(" %u", (unsigned)ob[(size_t)s * cap + i]);
        printf("\n");
    }
    rs_destroy(ctx);
    for (void* p : {d_kps, d_poses, d_start, d_obs, d_world, d_matches, d_nmatches, d_best, d_pose, d_best_id, d_inliers, d_n_inliers, d_out})
        (void)hipFree(p);
    printf("single_view ok\n");
    return 0;
}
