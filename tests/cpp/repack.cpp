// repack.cpp — cv_sfm::TableRepack of include/akaze.hpp from a native process (no Python, no PyTorch) linked to libakz.so: one
// landmark table, one block map and one pool read from a file, device buffers from hipMalloc, the repacked table and the
// gathered pool, every output printed.
// usage: repack call.bin
// call.bin: u32 {n_blocks, cap, n_landmarks, n_obs, n_blocks_out, has_map, lm_room, obs_room, row_words}, u32 obs_start
//           [n_landmarks + 1], u32 obs [n_obs][2], u32 map [n_blocks], u32 pool [n_blocks][row_words]
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

static bool take(FILE* fp, std::vector<uint32_t>& dst)
{
    return dst.empty() || fread(dst.data(), sizeof(uint32_t), dst.size(), fp) == dst.size();
}

static hipError_t upload(const std::vector<uint32_t>& src, void** d)
{
    hipError_t e = hipMalloc(d, sizeof(uint32_t) * (src.empty() ? 1 : src.size()));
    if (e == hipSuccess && !src.empty()) e = hipMemcpy(*d, src.data(), sizeof(uint32_t) * src.size(), hipMemcpyHostToDevice);
    return e;
}

// a device buffer of n words, every word 0xA5A5A5A5 so that an unwritten one shows
static hipError_t poisoned(size_t n, void** d)
{
    hipError_t e = hipMalloc(d, sizeof(uint32_t) * (n ? n : 1));
    if (e == hipSuccess) e = hipMemset(*d, 0xA5, sizeof(uint32_t) * (n ? n : 1));
    return e;
}

static int show(const char* name, const void* d, size_t n)
{
    std::vector<uint32_t> v(n ? n : 1);
    HIPOK(hipMemcpy(v.data(), d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
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
    std::vector<uint32_t> head(9);
    if (!take(fp, head)) return 2;
    const uint32_t n_blocks = head[0], cap = head[1], n_lm = head[2], n_obs = head[3], n_out = head[4], lm_room = head[6], obs_room = head[7],
                   row_words = head[8];
    const bool has_map = head[5] != 0;
    std::vector<uint32_t> start((size_t)n_lm + 1), obs(2 * (size_t)n_obs), map(n_blocks), pool((size_t)n_blocks * row_words);
    if (!take(fp, start) || !take(fp, obs) || !take(fp, map) || !take(fp, pool)) return 2;
    fclose(fp);
    if (cv_sfm::TableRepack::room(n_out, cap) > 0xFFFFFFFEull) return 2;

    void *d_start, *d_obs, *d_map, *d_pool, *d_start_out, *d_obs_out, *d_obs_counts, *d_landmarks, *d_key, *d_counts, *d_verdict, *d_pool_out,
        *d_pool_verdict;
    HIPOK(upload(start, &d_start));
    HIPOK(upload(obs, &d_obs));
    HIPOK(upload(map, &d_map));
    HIPOK(upload(pool, &d_pool));
    HIPOK(poisoned((size_t)lm_room + 1, &d_start_out));
    HIPOK(poisoned(2 * (size_t)obs_room, &d_obs_out));
    HIPOK(poisoned(lm_room, &d_obs_counts));
    HIPOK(poisoned((size_t)n_out * cap, &d_landmarks));
    HIPOK(poisoned(n_lm, &d_key));
    HIPOK(poisoned(RS_RP_COUNTS, &d_counts));
    HIPOK(poisoned(1, &d_verdict));
    HIPOK(poisoned((size_t)n_out * row_words, &d_pool_out));
    HIPOK(poisoned(1, &d_pool_verdict));
    try {
        cv_sfm::TableRepack repack(0);
        repack.table(d_start, d_obs, n_obs, n_lm, cap, n_blocks, has_map ? d_map : nullptr, n_out, nullptr, 0, obs_room, lm_room, d_start_out,
                     d_obs_out, d_obs_counts, d_landmarks, d_key, nullptr, d_counts, d_verdict);
        if (row_words) repack.gather(d_pool, d_pool_out, 4 * row_words, n_blocks, has_map ? d_map : nullptr, n_out, d_pool_verdict);
        repack.sync();
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    if (show("verdict", d_verdict, 1) || show("counts", d_counts, RS_RP_COUNTS) || show("obs_start_out", d_start_out, (size_t)lm_room + 1) ||
        show("obs_out", d_obs_out, 2 * (size_t)obs_room) || show("obs_counts_out", d_obs_counts, lm_room) ||
        show("landmarks_out", d_landmarks, (size_t)n_out * cap) || show("key_out", d_key, n_lm))
        return 4;
    if (row_words && (show("pool_verdict", d_pool_verdict, 1) || show("pool_out", d_pool_out, (size_t)n_out * row_words))) return 4;
    return 0;
}
