// landmark_table.cpp — cv_sfm::LandmarkBook of include/akaze.hpp from a native process (no Python, no PyTorch) linked to libakz.so:
// one landmark table and one micro-batch read from a file, device buffers from hipMalloc, the mask of the merge candidates and the
// next generation of the table, every output printed.
// usage: landmark_table call.bin
// call.bin: u32 {n_blocks, cap, n_landmarks, n_obs, n_world, n_frames, split_room, has_best}, u32 obs_start [n_landmarks + 1],
//           u32 obs [n_obs][2], u32 split [split_room][2], u32 split_count [1], u32 ik [n_frames], u32 counts [n_blocks],
//           u32 matches [n_frames][cap][2], u32 nmatches [n_frames], u32 verdict [n_frames], u32 best [n_frames][cap][3][2],
//           u32 decision [n_frames][cap], f64 pose_out [n_frames][12], u8 final [n_frames][cap]
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
static void show(const char* name, const T* v, size_t n)
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
    std::vector<uint32_t> head(8);
    if (!take(fp, head)) return 2;
    const uint32_t n_blocks = head[0], cap = head[1], n_lm = head[2], n_obs = head[3], n_world = head[4], F = head[5], split_room = head[6];
    const bool has_best = head[7] != 0;
    const size_t slots = (size_t)F * cap;
    std::vector<uint32_t> start((size_t)n_lm + 1), obs(2 * (size_t)n_obs), split(2 * (size_t)split_room), split_count(1), ik(F), counts(n_blocks),
        matches(2 * slots), nmatches(F), verdict(F), best(6 * slots), decision(slots);
    std::vector<double> pose_out(12 * (size_t)F), poses(12 * (size_t)n_blocks, -1.0);
    std::vector<unsigned char> final_mask(slots);
    if (!take(fp, start) || !take(fp, obs) || !take(fp, split) || !take(fp, split_count) || !take(fp, ik) || !take(fp, counts) ||
        !take(fp, matches) || !take(fp, nmatches) || !take(fp, verdict) || !take(fp, best) || !take(fp, decision) || !take(fp, pose_out) ||
        !take(fp, final_mask))
        return 2;
    fclose(fp);

    const uint64_t obs_room64 = cv_sfm::LandmarkBook::room(n_obs, split_room, F, cap), lm_room64 = cv_sfm::LandmarkBook::room(n_lm, split_room, F, cap);
    if (obs_room64 > 0xFFFFFFFFull || lm_room64 >= 0xFFFFFFFFull) return 2;
    const uint32_t obs_room = (uint32_t)obs_room64, lm_room = (uint32_t)lm_room64;
    void *d_start, *d_obs, *d_split, *d_split_count, *d_counts, *d_matches, *d_nmatches, *d_verdict, *d_best, *d_decision, *d_pose_out, *d_final,
        *d_poses, *d_out, *d_mask;
    HIPOK(upload(start, &d_start));
    HIPOK(upload(obs, &d_obs));
    HIPOK(upload(split, &d_split));
    HIPOK(upload(split_count, &d_split_count));
    HIPOK(upload(counts, &d_counts));
    HIPOK(upload(matches, &d_matches));
    HIPOK(upload(nmatches, &d_nmatches));
    HIPOK(upload(verdict, &d_verdict));
    HIPOK(upload(best, &d_best));
    HIPOK(upload(decision, &d_decision));
    HIPOK(upload(pose_out, &d_pose_out));
    HIPOK(upload(final_mask, &d_final));
    HIPOK(upload(poses, &d_poses));
    // one buffer for every word the call writes
    const size_t lm_words = (size_t)n_blocks * cap;
    const size_t n_words = ((size_t)lm_room + 1) + 2 * ((size_t)obs_room + 1) + RS_AV_COUNTS + lm_words + ((size_t)lm_room + 1) + (F + 1) +
                           (size_t)RS_AV_STATS * (F + 1) + 1;
    HIPOK(hipMalloc(&d_out, 4 * n_words));
    HIPOK(hipMemset(d_out, 0xA5, 4 * n_words));
    HIPOK(hipMalloc(&d_mask, slots ? slots : 1));
    HIPOK(hipMemset(d_mask, 0xA5, slots ? slots : 1));
    uint32_t* w = static_cast<uint32_t*>(d_out);
    uint32_t *d_start_out = w, *d_obs_out = d_start_out + lm_room + 1, *d_counts_out = d_obs_out + 2 * ((size_t)obs_room + 1),
             *d_landmarks_out = d_counts_out + RS_AV_COUNTS, *d_obs_counts_out = d_landmarks_out + lm_words,
             *d_frame_verdict = d_obs_counts_out + lm_room + 1, *d_stats = d_frame_verdict + F + 1,
             *d_call_verdict = d_stats + (size_t)RS_AV_STATS * (F + 1);
    try {
        cv_sfm::LandmarkBook book;
        book.sharing_view(d_start, d_obs, n_obs, n_lm, d_best, d_decision, cap, F, d_mask);
        book.add_views(d_start, d_obs, n_obs, n_lm, n_world, split_room ? d_split : nullptr, split_room ? d_split_count : nullptr, split_room, cap,
                       n_blocks, ik, d_counts, d_matches, d_nmatches, d_final, d_verdict, d_pose_out, has_best ? d_best : nullptr, nullptr,
                       obs_room, lm_room, d_poses, d_start_out, d_obs_out, d_counts_out, d_landmarks_out, d_obs_counts_out, d_frame_verdict,
                       d_stats, d_call_verdict);
        book.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    std::vector<uint32_t> ow(n_words);
    std::vector<unsigned char> mask(slots ? slots : 1);
    HIPOK(hipMemcpy(ow.data(), w, 4 * n_words, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(mask.data(), d_mask, mask.size(), hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(poses.data(), d_poses, sizeof(double) * poses.size(), hipMemcpyDeviceToHost));
    const uint32_t* h = ow.data();
    const uint32_t* counts_out = h + (d_counts_out - w);
    show("mask", mask.data(), slots);
    show("counts", counts_out, RS_AV_COUNTS);
    show("start", h, (size_t)counts_out[0] + 1);
    show("obs", h + (d_obs_out - w), 2 * (size_t)counts_out[1]);
    show("landmarks", h + (d_landmarks_out - w), lm_words);
    show("obs_counts", h + (d_obs_counts_out - w), counts_out[0]);
    show("verdicts", h + (d_frame_verdict - w), F);
    show("stats", h + (d_stats - w), (size_t)RS_AV_STATS * F);
    show("call", h + (d_call_verdict - w), 1);
    printf("poses");
    for (double v : poses) printf(" %.17g", v);
    printf("\n");
    for (void* p : {d_start, d_obs, d_split, d_split_count, d_counts, d_matches, d_nmatches, d_verdict, d_best, d_decision, d_pose_out, d_final,
                    d_poses, d_out, d_mask})
        (void)hipFree(p);
    printf("landmark_table ok\n");
    return 0;
}
