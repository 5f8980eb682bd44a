// export.cpp — cv_sfm::ReconstructionExport of include/akaze.hpp from a native process (no Python, no PyTorch) linked to
// libakz.so: a reconstruction read from a file, device buffers from hipMalloc, the export, the .ply file written from the rows
// the call filled, the counts and the verdict printed.
// usage: export call.bin out.ply
// call.bin: u32 {n_world, n_landmarks, n_obs, n_blocks, cap, n_views, room, camera_faces},
//           f64 world [n_world][4], u32 start [n_landmarks + 1], u32 obs [n_obs][2], u8 colors [n_blocks][cap][3],
//           u32 view_blocks [n_views], u32 counts [n_blocks], u32 landmarks [n_blocks][cap], f64 poses [n_blocks][12]
#include <hip/hip_runtime_api.h>

#include <algorithm>
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
    if (argc != 3) return 2;
    FILE* fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    std::vector<uint32_t> head(8);
    if (!take(fp, head)) return 2;
    const uint32_t n_world = head[0], n_landmarks = head[1], n_obs = head[2], n_blocks = head[3], cap = head[4], n_views = head[5], room = head[6];
    const bool camera_faces = head[7] != 0;
    std::vector<double> world(4 * (size_t)n_world), poses(12 * (size_t)n_blocks);
    std::vector<uint32_t> start((size_t)n_landmarks + 1), obs(2 * (size_t)n_obs), view_blocks(n_views), counts(n_blocks), landmarks((size_t)n_blocks * cap);
    std::vector<uint8_t> colors(3 * (size_t)n_blocks * cap);
    if (!take(fp, world) || !take(fp, start) || !take(fp, obs) || !take(fp, colors) || !take(fp, view_blocks) || !take(fp, counts) ||
        !take(fp, landmarks) || !take(fp, poses))
        return 2;
    fclose(fp);

    const size_t n_vertices = (size_t)RS_EX_CAMERA_VERTICES * n_views + room;
    void *d_world, *d_start, *d_obs, *d_colors, *d_counts, *d_landmarks, *d_poses, *d_xyz, *d_rgb, *d_key, *d_cameras, *d_words;
    HIPOK(upload(world, &d_world));
    HIPOK(upload(start, &d_start));
    HIPOK(upload(obs, &d_obs));
    HIPOK(upload(colors, &d_colors));
    HIPOK(upload(counts, &d_counts));
    HIPOK(upload(landmarks, &d_landmarks));
    HIPOK(upload(poses, &d_poses));
    HIPOK(hipMalloc(&d_xyz, sizeof(double) * 3 * (n_vertices + 1)));
    HIPOK(hipMalloc(&d_rgb, 3 * (n_vertices + 1)));
    HIPOK(hipMalloc(&d_key, sizeof(uint32_t) * ((size_t)room + 1)));
    HIPOK(hipMalloc(&d_cameras, sizeof(double) * RS_EX_CAMERA_WORDS * ((size_t)n_views + 1)));
    HIPOK(hipMalloc(&d_words, sizeof(uint32_t) * (RS_EX_COUNTS + 1)));
    uint32_t* d_counts_out = static_cast<uint32_t*>(d_words);
    try {
        cv_sfm::ReconstructionExport ex;
        ex.export_device(d_world, n_world, d_start, d_obs, n_obs, n_landmarks, d_colors, view_blocks, d_counts, d_landmarks, cap, n_blocks, d_poses,
                         room, d_xyz, d_rgb, d_key, d_cameras, d_counts_out, d_counts_out + RS_EX_COUNTS);
        ex.sync();
        uint32_t words[RS_EX_COUNTS + 1];
        HIPOK(hipMemcpy(words, d_words, sizeof(words), hipMemcpyDeviceToHost));
        const size_t used = (size_t)RS_EX_CAMERA_VERTICES * n_views + std::min(words[RS_EX_C_POINTS], room);
        std::vector<double> xyz(3 * used);
        std::vector<uint8_t> rgb(3 * used);
        HIPOK(hipMemcpy(xyz.data(), d_xyz, sizeof(double) * xyz.size(), hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(rgb.data(), d_rgb, rgb.size(), hipMemcpyDeviceToHost));
        cv_sfm::ReconstructionExport::write_ply(argv[2], xyz, rgb, n_views, camera_faces);
        printf("counts %u %u %u %u\nverdict %u\n", words[0], words[1], words[2], words[3], words[RS_EX_COUNTS]);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    for (void* p : {d_world, d_start, d_obs, d_colors, d_counts, d_landmarks, d_poses, d_xyz, d_rgb, d_key, d_cameras, d_words}) (void)hipFree(p);
    printf("export ok\n");
    return 0;
}
