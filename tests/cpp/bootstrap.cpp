// bootstrap.cpp — cv_sfm::ReconstructionStart of include/akaze.hpp from a native process (no Python, no PyTorch) linked to
// libakz.so: the slots of one consensus call and the masks of one bootstrap call read from a file, device buffers from
// hipMalloc, the join and then add_reconstruction over the join's lists, every output printed.
// usage: bootstrap call.bin
// call.bin: u32 {n_slots, cap, n_scenes, n_src_blocks, n_blocks, view_base, minimum, flags, seed low, seed high},
//           u32 pairs [n_slots][cap][2], npairs [n_slots], inliers [n_slots][cap], n_inliers [n_slots], best_id [n_slots],
//           slot_first, slot_second, ic, i_first, i_second, tv_verdict [n_scenes], counts [n_src_blocks],
//           f64 pose [n_slots][12], pose_out [n_scenes][24], u8 combined, first_ok, second_ok [n_scenes][cap],
//           kps [n_src_blocks][cap][28]
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

static hipError_t filled(size_t bytes, void** d)
{
    hipError_t e = hipMalloc(d, bytes ? bytes : 1);
    return e == hipSuccess ? hipMemset(*d, 0xA5, bytes ? bytes : 1) : e;
}

static int show(const char* name, const void* d, size_t n)
{
    std::vector<uint32_t> v(n ? n : 1);
    HIPOK(hipMemcpy(v.data(), d, 4 * n, hipMemcpyDeviceToHost));
    printf("%s", name);
    for (size_t i = 0; i < n; ++i) printf(" %u", (unsigned)v[i]);
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint32_t> head(10);
    if (!take(fp, head)) return 2;
    const uint32_t n_slots = head[0], cap = head[1], S = head[2], n_src = head[3], n_blocks = head[4], view_base = head[5], minimum = head[6],
                   flags = head[7];
    const uint64_t seed = (uint64_t)head[8] | ((uint64_t)head[9] << 32);
    const size_t slot_words = (size_t)n_slots * cap, scene_words = (size_t)S * cap;
    std::vector<uint32_t> pairs(2 * slot_words), npairs(n_slots), inliers(slot_words), n_inliers(n_slots), best_id(n_slots), slot_first(S),
        slot_second(S), ic(S), i_first(S), i_second(S), tv_verdict(S), counts(n_src);
    std::vector<double> pose(12 * (size_t)n_slots), pose_out(24 * (size_t)S);
    std::vector<unsigned char> combined(scene_words), first_ok(scene_words), second_ok(scene_words), kps((size_t)n_src * cap * 28);
    if (!take(fp, pairs) || !take(fp, npairs) || !take(fp, inliers) || !take(fp, n_inliers) || !take(fp, best_id) || !take(fp, slot_first) ||
        !take(fp, slot_second) || !take(fp, ic) || !take(fp, i_first) || !take(fp, i_second) || !take(fp, tv_verdict) || !take(fp, counts) ||
        !take(fp, pose) || !take(fp, pose_out) || !take(fp, combined) || !take(fp, first_ok) || !take(fp, second_ok) || !take(fp, kps))
        return 2;
    fclose(fp);

    const uint32_t room = 3 * S * cap;
    void *d_pairs, *d_npairs, *d_inliers, *d_n_inliers, *d_best_id, *d_pose, *d_tv, *d_counts, *d_pose_out, *d_combined, *d_first_ok, *d_second_ok,
        *d_kps, *d_triples, *d_first, *d_second, *d_n, *d_pf, *d_ps, *d_jv, *d_kps_dst, *d_counts_dst, *d_poses, *d_start, *d_obs, *d_obs_counts,
        *d_counts_out, *d_landmarks, *d_recon, *d_view, *d_views, *d_cposes, *d_cverdict, *d_fv, *d_stats, *d_call;
    HIPOK(upload(pairs, &d_pairs));
    HIPOK(upload(npairs, &d_npairs));
    HIPOK(upload(inliers, &d_inliers));
    HIPOK(upload(n_inliers, &d_n_inliers));
    HIPOK(upload(best_id, &d_best_id));
    HIPOK(upload(pose, &d_pose));
    HIPOK(upload(tv_verdict, &d_tv));
    HIPOK(upload(counts, &d_counts));
    HIPOK(upload(pose_out, &d_pose_out));
    HIPOK(upload(combined, &d_combined));
    HIPOK(upload(first_ok, &d_first_ok));
    HIPOK(upload(second_ok, &d_second_ok));
    HIPOK(upload(kps, &d_kps));
    HIPOK(filled(12 * scene_words, &d_triples));
    HIPOK(filled(8 * scene_words, &d_first));
    HIPOK(filled(8 * scene_words, &d_second));
    HIPOK(filled(4 * 3 * (size_t)S, &d_n));
    HIPOK(filled(96 * (size_t)S, &d_pf));
    HIPOK(filled(96 * (size_t)S, &d_ps));
    HIPOK(filled(4 * (size_t)S, &d_jv));
    HIPOK(filled((size_t)n_blocks * cap * 28, &d_kps_dst));
    HIPOK(filled(4 * (size_t)n_blocks, &d_counts_dst));
    HIPOK(filled(96 * (size_t)n_blocks, &d_poses));
    HIPOK(filled(4 * ((size_t)room + 1), &d_start));
    HIPOK(filled(8 * (size_t)room, &d_obs));
    HIPOK(filled(4 * (size_t)room, &d_obs_counts));
    HIPOK(filled(4 * RS_AR_COUNTS, &d_counts_out));
    HIPOK(filled(4 * (size_t)n_blocks * cap, &d_landmarks));
    HIPOK(filled(4 * ((size_t)S + 1), &d_recon));
    HIPOK(filled(4 * ((size_t)S + 1), &d_view));
    HIPOK(filled(12 * (size_t)S, &d_views));
    HIPOK(filled(192 * (size_t)S, &d_cposes));
    HIPOK(filled(4 * (size_t)S, &d_cverdict));
    HIPOK(filled(4 * (size_t)S, &d_fv));
    HIPOK(filled(4 * RS_AR_STATS * (size_t)S, &d_stats));
    HIPOK(filled(4, &d_call));
    uint32_t* n = static_cast<uint32_t*>(d_n);
    try {
        cv_sfm::ReconstructionStart start;
        start.join_pairs_device(d_pairs, d_npairs, d_inliers, d_n_inliers, d_best_id, d_pose, n_slots, cap, slot_first, slot_second, minimum, flags,
                                seed, d_triples, n, d_first, n + S, d_second, n + 2 * (size_t)S, d_pf, d_ps, d_jv);
        start.add_reconstruction_device(d_triples, n, d_first, n + S, d_second, n + 2 * (size_t)S, d_combined, d_first_ok, d_second_ok, d_pose_out,
                                        d_tv, ic, i_first, i_second, d_kps, d_counts, n_src, cap, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr,
                                        0, d_kps_dst, d_counts_dst, d_poses, n_blocks, view_base, room, room, d_start, d_obs, d_obs_counts,
                                        d_counts_out, d_landmarks, d_recon, d_view, d_views, d_cposes, d_cverdict, d_fv, d_stats, d_call);
        start.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    uint32_t filled_counts[RS_AR_COUNTS];
    HIPOK(hipMemcpy(filled_counts, d_counts_out, sizeof filled_counts, hipMemcpyDeviceToHost));
    if (show("join_counts", d_n, 3 * (size_t)S) || show("join_verdict", d_jv, S) || show("triples", d_triples, 3 * scene_words) ||
        show("counts", d_counts_out, RS_AR_COUNTS) || show("start", d_start, (size_t)filled_counts[0] + 1) ||
        show("obs", d_obs, 2 * (size_t)filled_counts[1]) || show("obs_counts", d_obs_counts, filled_counts[0]) ||
        show("landmarks", d_landmarks, (size_t)n_blocks * cap) || show("recon_start", d_recon, (size_t)S + 1) ||
        show("view_start", d_view, (size_t)S + 1) || show("views", d_views, 3 * (size_t)S) || show("constraint_verdict", d_cverdict, S) ||
        show("verdicts", d_fv, S) || show("stats", d_stats, (size_t)RS_AR_STATS * S) || show("call", d_call, 1) ||
        show("counts_dst", d_counts_dst, n_blocks) || show("kps_dst", d_kps_dst, (size_t)n_blocks * cap * 7))
        return 4;
    std::vector<double> poses(12 * (size_t)n_blocks);
    HIPOK(hipMemcpy(poses.data(), d_poses, sizeof(double) * poses.size(), hipMemcpyDeviceToHost));
    printf("poses");
    for (double v : poses) printf(" %.17g", v);
    printf("\n");
    for (void* p : {d_pairs, d_npairs, d_inliers, d_n_inliers, d_best_id, d_pose, d_tv, d_counts, d_pose_out, d_combined, d_first_ok, d_second_ok,
                    d_kps, d_triples, d_first, d_second, d_n, d_pf, d_ps, d_jv, d_kps_dst, d_counts_dst, d_poses, d_start, d_obs, d_obs_counts,
                    d_counts_out, d_landmarks, d_recon, d_view, d_views, d_cposes, d_cverdict, d_fv, d_stats, d_call})
        (void)hipFree(p);
    printf("bootstrap ok\n");
    return 0;
}
