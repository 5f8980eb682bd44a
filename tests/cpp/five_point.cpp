// five_point.cpp — Consensus::model_inliers(&NisterStewenius::new(), matches) through the C++ host-side mirror
// (include/akaze.hpp), i.e. through the C ABI of libakz.so, from a native process.
// usage: five_point matches.bin out.bin threshold seed n_hypotheses block_size
//   matches.bin  n x 6 f64: unit bearings a, b of every match
//   out.bin      u32 found, u32 n_inliers, 12 f64 pose, then n_inliers u32 inlier indices — the bytes the ctypes path gives
// The builder is set to the bound alone (no cap, no SPRT, no re-sampling): tests/test_gpu_five_point.py runs
// rs_essential_arrsac with the same parameters and compares the files.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "akaze.hpp"

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<cv_core::FeatureMatch> matches;
    double row[6];
    while (fread(row, sizeof(double), 6, f) == 6) matches.push_back(cv_core::FeatureMatch{{row[0], row[1], row[2]}, {row[3], row[4], row[5]}});
    fclose(f);
    try {
        auto arrsac = arrsac::Arrsac(atof(argv[3]), strtoull(argv[4], nullptr, 10))
                          .initialization_hypotheses((uint32_t)atoi(argv[5]))
                          .block_size((uint32_t)atoi(argv[6]))
                          .initialization_blocks(1)
                          .max_candidate_hypotheses(0)
                          .estimations_per_block(0)
                          .likelihood_ratio_threshold(1e300);
        auto r = arrsac.model_inliers(nister_stewenius::NisterStewenius{}, matches);
        // fewer than MIN_SAMPLES matches: None, without touching the device
        std::vector<cv_core::FeatureMatch> four(matches.begin(), matches.begin() + (matches.size() < 4 ? matches.size() : 4));
        if (arrsac.model_inliers(nister_stewenius::NisterStewenius{}, four)) {
            fprintf(stderr, "four matches gave a model\n");
            return 1;
        }
        FILE* o = fopen(argv[2], "wb");
        if (!o) return 2;
        uint32_t head[2] = {r ? 1u : 0u, r ? (uint32_t)r->second.size() : 0u};
        fwrite(head, sizeof(uint32_t), 2, o);
        if (r) {
            fwrite(r->first.rt.data(), sizeof(double), 12, o);
            for (std::size_t i : r->second) {
                const uint32_t v = (uint32_t)i;
                fwrite(&v, sizeof(uint32_t), 1, o);
            }
        }
        fclose(o);
        printf("five_point ok: %u inliers of %zu\n", head[1], matches.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
