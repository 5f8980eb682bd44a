// akaze.hpp — C++ host-side mirror of the reference's Rust API for the hot path, over the C ABI
// of akz.h.  The reference's own toolchain (cargo/rustc) is not available in the build image, so the
// host side above the C ABI is C++ (and ctypes for the tests); the Rust shim a maintainer would add is
// in INTEGRATION.md / rust/akaze-mi355x/.
//
// Same names, argument meaning and error behaviour as the reference (paths relative to rust-cv/cv):
//   akaze::Akaze            11 public fields, Default, new_/sparse/dense          akaze/src/lib.rs:109-185
//   Akaze::extract / extract_from_gray_float_image                                akaze/src/lib.rs:295, 309
//   akaze::KeyPoint         point, response, size, octave, class_id, angle        akaze/src/lib.rs:69-93
//   bitarray::BitArray<64>  64 descriptor bytes, bit i at bytes[i>>3] bit (i&7)   akaze/src/descriptors.rs:197
//   space::LinearKnn{metric: Hamming, iter}.knn(query, 2) -> [Neighbor; 2]        akaze/tests/estimate_pose.rs:82-88
//   matching / symmetric_matching                      tutorial-code/chapter5-geometric-verification/src/main.rs:154-200
//   match_descriptors (Lowe ratio)                                                akaze/tests/estimate_pose.rs:78-97
//
// Error behaviour: Akaze::extract is infallible in the reference (keypoints whose descriptor samples
// leave the image are silently dropped).  Here device problems (no GPU, out of memory, list overflow)
// additionally throw akaze::Error — there is no CPU fallback to fall back to.
#pragma once

#include <array>
#include <cstdint>
#include <cstring>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "akz.h"

namespace akaze {

struct Error : std::runtime_error {
    int32_t status;
    Error(int32_t s, const std::string& what) : std::runtime_error(what + ": " + akz_strerror(s)), status(s) {}
};
inline void check(int32_t s, const char* what)
{
    if (s != AKZ_OK) throw Error(s, what);
}
// The library this translation unit is linked to must export the ABI this header was written against (AKZ_ABI_VERSION).
inline void require_abi()
{
    static const bool ok = akz_abi_version() == AKZ_ABI_VERSION;
    if (!ok) throw std::runtime_error("libakz exports ABI " + std::to_string(akz_abi_version()) + ", akaze.hpp was written against " +
                                      std::to_string(AKZ_ABI_VERSION));
}

// akaze::KeyPoint (lib.rs:69-93)
struct KeyPoint {
    std::pair<float, float> point;
    float response;
    float size;
    std::size_t octave;
    std::size_t class_id;
    float angle;
    // cv_core::ImagePoint::image_point (lib.rs:95-99)
    std::pair<double, double> image_point() const { return {(double)point.first, (double)point.second}; }
};

using BitArray64 = std::array<uint8_t, 64>;  // bitarray::BitArray<64>

// A Luma8 image view (what DynamicImage::ImageLuma8 hands to GrayFloatImage::from_dynamic, image.rs:47-56).
struct GrayImageU8 {
    const uint8_t* data;
    int width, height, stride;
};
// A GrayFloatImage view (image.rs:36): f32 pixels in [0,1], row-major.
struct GrayFloatImage {
    const float* data;
    int width, height, stride;
};

// A colour image view (DynamicImage::ImageRgb8 / Rgba8: what image.rs:45-46 sends through grayscale() first).
struct ColorImageU8 {
    const uint8_t* data;
    int width, height, stride;   // stride in bytes
    int channels;                // 3 (RGB) or 4 (RGBA)
};

namespace detail {
// Device contexts are not part of akaze::Akaze (a Copy struct of eleven fields whose methods take &self and keep no
// state, lib.rs:108-142): they live in a small per-thread cache keyed by everything a context is created from, so that
// a loop of extract() calls — cv-sfm/src/lib.rs:2200-2204 — re-uses one pyramid instead of allocating ~0.2 GB per frame.
struct CtxKey {
    akz_config cfg;
    int device, w, h;
    uint32_t max_keypoints;
    uint32_t arith = 0;   // akz_options.arith (tools/pin_arith.py names the value a given Rust build computes)
    bool same(const CtxKey& o) const
    {
        return arith == o.arith && cfg.maximum_features == o.cfg.maximum_features && cfg.num_sublevels == o.cfg.num_sublevels &&
               cfg.max_octave_evolution == o.cfg.max_octave_evolution && cfg.base_scale_offset == o.cfg.base_scale_offset &&
               cfg.initial_contrast == o.cfg.initial_contrast && cfg.contrast_percentile == o.cfg.contrast_percentile &&
               cfg.contrast_factor_num_bins == o.cfg.contrast_factor_num_bins && cfg.derivative_factor == o.cfg.derivative_factor &&
               cfg.detector_threshold == o.cfg.detector_threshold && cfg.descriptor_channels == o.cfg.descriptor_channels &&
               cfg.descriptor_pattern_size == o.cfg.descriptor_pattern_size && device == o.device && max_keypoints == o.max_keypoints;
    }
};
struct CtxCache {
    static constexpr int kSlots = 2;
    struct Slot {
        CtxKey key;
        akz_ctx* ctx = nullptr;
        uint64_t used = 0;
    } slots[kSlots];
    uint64_t tick = 0;
    ~CtxCache()
    {
        for (Slot& s : slots)
            if (s.ctx) akz_destroy(s.ctx);
    }
    akz_ctx* get(const CtxKey& k)
    {
        for (Slot& s : slots)
            if (s.ctx && s.key.same(k) && k.w <= s.key.w && k.h <= s.key.h) {
                s.used = ++tick;
                return s.ctx;
            }
        Slot* victim = &slots[0];
        for (Slot& s : slots) {
            if (!s.ctx) {
                victim = &s;
                break;
            }
            if (s.used < victim->used) victim = &s;
        }
        if (victim->ctx) akz_destroy(victim->ctx);
        victim->ctx = nullptr;
        require_abi();
        akz_options opt = {};
        opt.struct_size = (uint32_t)sizeof(opt);
        opt.arith = k.arith;
        check(akz_create_ex(&k.cfg, k.device, k.w, k.h, 1, k.max_keypoints, k.arith ? &opt : nullptr, &victim->ctx), "akz_create_ex");
        victim->key = k;
        victim->used = ++tick;
        return victim->ctx;
    }
    void drop(akz_ctx* c)
    {
        for (Slot& s : slots)
            if (s.ctx == c) {
                akz_destroy(c);
                s.ctx = nullptr;
            }
    }
};
inline CtxCache& ctx_cache()
{
    static thread_local CtxCache cache;
    return cache;
}
}  // namespace detail

class Akaze {
public:
    // the reference's 11 public fields, same names and defaults (lib.rs:109-185)
    std::size_t maximum_features = std::numeric_limits<std::size_t>::max();
    uint32_t num_sublevels = 4;
    uint32_t max_octave_evolution = 4;
    double base_scale_offset = 1.6;
    double initial_contrast = 0.001;
    double contrast_percentile = 0.7;
    std::size_t contrast_factor_num_bins = 300;
    double derivative_factor = 1.5;
    double detector_threshold = 0.001;
    std::size_t descriptor_channels = 3;
    std::size_t descriptor_pattern_size = 10;
    // placement (not part of the reference struct)
    int device = 0;
    // first capacity of the device's per-frame lists.  The reference's Vecs are unbounded; a call that overflows the
    // capacity is repeated with twice as much (up to the library's 262 144 per frame), so this is a starting point only.
    uint32_t initial_keypoint_capacity = 16384;
    // which of the reference's three un-vendored arithmetic orders the filters and half_size use (akz_options.arith,
    // AKZ_ARITH_* bits; 0 = what the crate sources imply).  `python3 tools/pin_arith.py <rust>_kps.csv <rust>_descs.txt image`
    // names the value that reproduces a given cargo build byte for byte.
    uint32_t arith = 0;

    static Akaze new_(double threshold)  // Akaze::new (lib.rs:147-152); `new` is reserved in C++
    {
        Akaze a;
        a.detector_threshold = threshold;
        return a;
    }
    static Akaze sparse() { return new_(0.01); }    // lib.rs:157-159
    static Akaze dense() { return new_(0.0001); }   // lib.rs:164-166

    using Features = std::pair<std::vector<KeyPoint>, std::vector<BitArray64>>;

    // Akaze::extract on a Luma8 image (lib.rs:295)
    Features extract(const GrayImageU8& img) const
    {
        return run(img.width, img.height, [&](akz_ctx* c, akz_keypoint* k, akz_descriptor* d, uint32_t cap, uint32_t* n) {
            return akz_extract_gray_u8(c, img.data, img.width, img.height, img.stride, k, d, cap, n);
        });
    }
    // Akaze::extract on a colour image: DynamicImage::grayscale() first (image.rs:45-46), on the device
    Features extract(const ColorImageU8& img) const
    {
        return run(img.width, img.height, [&](akz_ctx* c, akz_keypoint* k, akz_descriptor* d, uint32_t cap, uint32_t* n) {
            return akz_extract_color(c, img.data, AKZ_FMT_U8, img.channels, img.width, img.height, img.stride, k, d, cap, n);
        });
    }
    // Akaze::extract_from_gray_float_image (lib.rs:309)
    Features extract_from_gray_float_image(const GrayFloatImage& img) const
    {
        return run(img.width, img.height, [&](akz_ctx* c, akz_keypoint* k, akz_descriptor* d, uint32_t cap, uint32_t* n) {
            return akz_extract_gray_f32(c, img.data, img.width, img.height, img.stride, k, d, cap, n);
        });
    }

    akz_config config() const
    {
        akz_config c;
        c.maximum_features = (uint64_t)maximum_features;
        c.num_sublevels = num_sublevels;
        c.max_octave_evolution = max_octave_evolution;
        c.base_scale_offset = base_scale_offset;
        c.initial_contrast = initial_contrast;
        c.contrast_percentile = contrast_percentile;
        c.contrast_factor_num_bins = (uint64_t)contrast_factor_num_bins;
        c.derivative_factor = derivative_factor;
        c.detector_threshold = detector_threshold;
        c.descriptor_channels = (uint64_t)descriptor_channels;
        c.descriptor_pattern_size = (uint64_t)descriptor_pattern_size;
        return c;
    }

private:
    // one call, with growth: AKZ_E_INTERNAL (a device list overflowed) and AKZ_E_CAPACITY (more keypoints than the output
    // arrays hold) both mean "not enough room" — the reference has no such thing, so the call is repeated with more
    template <typename Call>
    Features run(int w, int h, Call call) const
    {
        constexpr uint32_t kLibraryMax = 262144;
        uint32_t cap = initial_keypoint_capacity < 64 ? 64 : (initial_keypoint_capacity > kLibraryMax ? kLibraryMax : initial_keypoint_capacity);
        if ((uint64_t)maximum_features < cap) cap = (uint32_t)(maximum_features < 64 ? 64 : maximum_features);
        for (;;) {
            detail::CtxKey key{config(), device, w, h, cap, arith};
            akz_ctx* c = detail::ctx_cache().get(key);
            std::vector<akz_keypoint> k(cap);
            std::vector<akz_descriptor> d(cap);
            uint32_t n = 0;
            const int32_t st = call(c, k.data(), d.data(), cap, &n);
            if (st == AKZ_OK) return convert(k, d, n);
            if ((st == AKZ_E_INTERNAL || st == AKZ_E_CAPACITY) && cap < kLibraryMax) {
                detail::ctx_cache().drop(c);
                cap = cap * 2 > kLibraryMax ? kLibraryMax : cap * 2;
                continue;
            }
            check(st, "akz_extract");
        }
    }
    static Features convert(const std::vector<akz_keypoint>& k, const std::vector<akz_descriptor>& d, uint32_t n)
    {
        Features out;
        out.first.reserve(n);
        out.second.reserve(n);
        for (uint32_t i = 0; i < n; ++i) {
            out.first.push_back(KeyPoint{{k[i].x, k[i].y}, k[i].response, k[i].size, k[i].octave, k[i].class_id, k[i].angle});
            BitArray64 b;
            for (int j = 0; j < 64; ++j) b[j] = d[i].bytes[j];
            out.second.push_back(b);
        }
        return out;
    }
};

}  // namespace akaze

namespace space {

struct Hamming {};  // bitarray::Hamming metric marker

// space::Neighbor<u32>
struct Neighbor {
    std::size_t index;
    uint32_t distance;
};

class Matcher {
public:
    explicit Matcher(uint32_t max_descriptors = 16384, int device = 0)
    {
        akaze::require_abi();
        akaze::check(hm_create(device, max_descriptors, max_descriptors, &ctx_), "hm_create");
    }
    ~Matcher()
    {
        if (ctx_) hm_destroy(ctx_);
    }
    Matcher(const Matcher&) = delete;
    Matcher& operator=(const Matcher&) = delete;
    hm_ctx* handle() { return ctx_; }

private:
    hm_ctx* ctx_ = nullptr;
};

// space::LinearKnn { metric: Hamming, iter }: exact k-NN by scanning `iter` (the target descriptors).
// The reference's callers ask once per query descriptor (akaze/tests/estimate_pose.rs:82-88).  `iter` goes to the device
// once (hm_set_targets, on the first question) and stays there; every knn() is then one launch over the resident targets
// — still launch-bound (ask for whole frames with knn_batch() or match_descriptors() where the loop is yours), but no
// longer an upload of the whole target set per query.
class LinearKnn {
public:
    LinearKnn(Hamming, const std::vector<akaze::BitArray64>& iter, Matcher& m) : iter_(iter), m_(m) {}
    // Knn::knn(&self, query, 2): sorted by (distance, index); the lowest index wins ties.
    std::array<Neighbor, 2> knn(const akaze::BitArray64& query, std::size_t num) const
    {
        if (num != 2) throw std::invalid_argument("the MI355X matcher implements knn(query, 2)");
        akz_neighbor out[2];
        ask(&query, 1, 2, out);
        return {Neighbor{out[0].index, out[0].distance}, Neighbor{out[1].index, out[1].distance}};
    }

    // Knn::knn(&self, query, num) -> Vec<Neighbor> for num = 1..3 (cv-sfm/src/lib.rs:1474 asks for 3):
    // min(num, iter.len()) neighbours, as the reference returns.
    std::vector<Neighbor> knn_vec(const akaze::BitArray64& query, std::size_t num) const
    {
        if (num < 1 || num > 3) throw std::invalid_argument("the MI355X matcher implements knn(query, k) for k <= 3");
        akz_neighbor out[3];
        ask(&query, 1, (uint32_t)num, out);
        std::vector<Neighbor> r;
        for (std::size_t i = 0; i < num && i < iter_.size(); ++i) r.push_back(Neighbor{out[i].index, out[i].distance});
        return r;
    }
    // the same for every query in one launch: out[i * num + j] = j-th neighbour of queries[i]
    std::vector<Neighbor> knn_batch(const std::vector<akaze::BitArray64>& queries, std::size_t num) const
    {
        if (num < 1 || num > 3) throw std::invalid_argument("the MI355X matcher implements knn(query, k) for k <= 3");
        std::vector<akz_neighbor> out(queries.size() * num);
        if (!queries.empty()) ask(queries.data(), (uint32_t)queries.size(), (uint32_t)num, out.data());
        std::vector<Neighbor> r(out.size());
        for (std::size_t i = 0; i < out.size(); ++i) r[i] = Neighbor{out[i].index, out[i].distance};
        return r;
    }

private:
    void ask(const akaze::BitArray64* q, uint32_t nq, uint32_t k, akz_neighbor* out) const
    {
        const akz_descriptor* t = reinterpret_cast<const akz_descriptor*>(iter_.data());
        // upload unless the matcher still holds THIS object's upload (its generation number: another LinearKnn on the same
        // matcher, or any host-buffer call that took the staging buffer, changes it)
        if (generation_ == 0 || hm_targets_generation(m_.handle()) != generation_) {
            akaze::check(hm_set_targets(m_.handle(), t, (uint32_t)iter_.size()), "hm_set_targets");
            generation_ = hm_targets_generation(m_.handle());
        }
        akaze::check(hm_knn_targets(m_.handle(), reinterpret_cast<const akz_descriptor*>(q), nq, k, out), "hm_knn_targets");
    }
    const std::vector<akaze::BitArray64>& iter_;
    Matcher& m_;
    mutable uint64_t generation_ = 0;
};

inline std::vector<std::array<std::size_t, 2>> run_match(Matcher& m, const std::vector<akaze::BitArray64>& a,
                                                         const std::vector<akaze::BitArray64>& b, int rule,
                                                         uint32_t pu, float pf, bool symmetric)
{
    std::vector<uint32_t> pairs(2 * (a.size() + 1));
    uint32_t n = 0;
    akaze::check(hm_match(m.handle(), reinterpret_cast<const akz_descriptor*>(a.data()), (uint32_t)a.size(),
                          reinterpret_cast<const akz_descriptor*>(b.data()), (uint32_t)b.size(), rule, pu, pf,
                          symmetric ? 1 : 0, pairs.data(), (uint32_t)a.size() + 1, &n),
                 "hm_match");
    std::vector<std::array<std::size_t, 2>> out(n);
    for (uint32_t i = 0; i < n; ++i) out[i] = {pairs[2 * i], pairs[2 * i + 1]};
    return out;
}
// symmetric_matching of tutorial ch5 (main.rs:183-200): keep [a, b] iff d0 + 24 < d1 both ways.
inline std::vector<std::array<std::size_t, 2>> symmetric_matching(Matcher& m, const std::vector<akaze::BitArray64>& a,
                                                                  const std::vector<akaze::BitArray64>& b)
{
    return run_match(m, a, b, HM_RULE_BETTER_BY_STRICT, 24, 0.f, true);
}
// match_descriptors of akaze/tests/estimate_pose.rs:78-97: a -> b only, Lowe ratio in f32.
inline std::vector<std::array<std::size_t, 2>> match_descriptors(Matcher& m, const std::vector<akaze::BitArray64>& ds1,
                                                                 const std::vector<akaze::BitArray64>& ds2,
                                                                 float lowes_ratio = 0.5f)
{
    return run_match(m, ds1, ds2, HM_RULE_LOWE, 0, lowes_ratio, false);
}

}  // namespace space

// ---- two-view / registration consensus: the sample_consensus::Consensus surface over rs_* -------------------------
//   cv_core::FeatureMatch(a, b) / FeatureWorldMatch(bearing, world)        cv-core/src/matches.rs
//   cv_pinhole::CameraIntrinsics::calibrate                                 cv-pinhole/src/lib.rs:108-117
//   eight_point::EightPoint, lambda_twist::LambdaTwist (Estimator)          eight-point/src/lib.rs:60-83, lambda-twist/src/lib.rs:330-347
//   nister_stewenius::NisterStewenius (Estimator)                           nister-stewenius/src/lib.rs:283-330
//   arrsac::Arrsac::{new, initialization_hypotheses, max_candidate_hypotheses, estimations_per_block, block_size,
//                    likelihood_ratio_threshold} + Consensus::{model, model_inliers}
//                                                                           call sites akaze/tests/estimate_pose.rs:63-75,
//                                                                           vslam-sandbox/src/main.rs:105-117, cv-sfm/src/lib.rs:1394-1412
// The arrsac crate is not vendored in the reference: what runs is this library's ARRSAC-shaped procedure (include/akz.h:
// rs_essential_arrsac / rs_p3p_arrsac, specified by oracle/arrsac_oracle.c); the builder names are the crate's.
namespace cv_core {
struct FeatureMatch {
    std::array<double, 3> a, b;       // unit bearings of the two views
};
struct FeatureWorldMatch {
    std::array<double, 3> bearing;    // unit bearing in the camera
    std::array<double, 4> world;      // homogeneous world point (Projective form: xyz normalised, w = 1 / distance)
};
struct CameraToCamera {
    std::array<double, 12> rt;        // row-major 3 x 4 [R | t]
};
struct WorldToCamera {
    std::array<double, 12> rt;
};
}  // namespace cv_core

namespace cv_pinhole {
struct CameraIntrinsics {
    std::array<double, 2> focals, principal_point;
    double skew = 0.0;
    // CameraModel::calibrate (lib.rs:108-117): pixel keypoint -> unit bearing
    std::array<double, 3> calibrate(const akaze::KeyPoint& kp) const
    {
        const double intr[5] = {focals[0], focals[1], principal_point[0], principal_point[1], skew};
        akz_keypoint k{};
        k.x = kp.point.first;
        k.y = kp.point.second;
        std::array<double, 3> out{};
        akaze::check(rs_calibrate(intr, 0, 0.0, &k, 1, out.data()), "rs_calibrate");
        return out;
    }
};
}  // namespace cv_pinhole

namespace eight_point {
struct EightPoint {
    static constexpr std::size_t MIN_SAMPLES = 8;   // eight-point/src/lib.rs:73
};
}  // namespace eight_point
namespace lambda_twist {
struct LambdaTwist {
    static constexpr std::size_t MIN_SAMPLES = 3;   // lambda-twist/src/lib.rs:333
};
}  // namespace lambda_twist
namespace nister_stewenius {
// The five-point minimal solver for calibrated cameras.  What runs is include/akz_five_point_math.h: the reference's
// algorithm with rows 6..9 of the action matrix's eigenvector (rows 5..8 as written at lib.rs:230 do not solve the problem).
struct NisterStewenius {
    static constexpr std::size_t MIN_SAMPLES = 5;   // nister-stewenius/src/lib.rs:308
};
}  // namespace nister_stewenius

namespace arrsac {

class Arrsac {
public:
    // Arrsac::new(inlier_threshold, rng): the rng is a seed here (the sampler is the library's xoshiro256++ streams)
    Arrsac(double inlier_threshold, uint64_t seed = 0, int device = 0) : device_(device)
    {
        std::memset(&p_, 0, sizeof(p_));
        p_.struct_size = sizeof(p_);
        // the defaults of arrsac 0.10's Arrsac::new as the crate documents them (un-vendored: not verifiable here) —
        // max_candidate_hypotheses 50, block_size 100, likelihood_ratio_threshold 1e3, initialization_hypotheses 256,
        // initialization_blocks 4, estimations_per_block 64 — so a caller ported with the bare constructor
        // (akaze/tests/estimate_pose.rs:63) runs the shape it ran before, inlier-guided re-sampling included
        p_.n_hypotheses = 256;
        p_.block_size = 100;
        p_.init_blocks = 4;
        p_.max_candidates = 50;
        p_.flags = RS_PRUNE_BOUND | RS_PRUNE_SPRT | RS_PRUNE_HALVE;
        p_.threshold = inlier_threshold;
        p_.sprt_delta = 0.05;
        p_.sprt_ratio = 1e3;
        p_.seed = seed;
        p_.estimations_per_block = 64;
    }
    ~Arrsac()
    {
        if (ctx_) rs_destroy(ctx_);
    }
    Arrsac(const Arrsac&) = delete;
    Arrsac& operator=(const Arrsac&) = delete;
    Arrsac(Arrsac&& o) noexcept : p_(o.p_), device_(o.device_), ctx_(o.ctx_), cap_m_(o.cap_m_), cap_h_(o.cap_h_) { o.ctx_ = nullptr; }

    // the crate's builder methods (vslam-sandbox/src/main.rs:105-117)
    Arrsac&& initialization_hypotheses(uint32_t n) && { p_.n_hypotheses = n; return std::move(*this); }
    Arrsac&& max_candidate_hypotheses(uint32_t n) && { p_.max_candidates = n; return std::move(*this); }
    Arrsac&& estimations_per_block(uint32_t n) && { p_.estimations_per_block = n; return std::move(*this); }
    Arrsac&& block_size(uint32_t n) && { p_.block_size = n; return std::move(*this); }
    Arrsac&& initialization_blocks(uint32_t n) && { p_.init_blocks = n; return std::move(*this); }
    Arrsac&& likelihood_ratio_threshold(double r) && { p_.sprt_ratio = r; return std::move(*this); }

    // Consensus<EightPoint, FeatureMatch>::model_inliers (eight-point/src/lib.rs:70-83 estimates, cv-core/src/pose.rs:249-295 scores)
    std::optional<std::pair<cv_core::CameraToCamera, std::vector<std::size_t>>> model_inliers(const eight_point::EightPoint&,
                                                                                              const std::vector<cv_core::FeatureMatch>& data)
    {
        if (data.size() < eight_point::EightPoint::MIN_SAMPLES) return std::nullopt;
        std::vector<double> a(3 * data.size()), b(3 * data.size());
        for (std::size_t i = 0; i < data.size(); ++i)
            for (int k = 0; k < 3; ++k) {
                a[3 * i + k] = data[i].a[k];
                b[3 * i + k] = data[i].b[k];
            }
        cv_core::CameraToCamera pose{};
        std::vector<std::size_t> inl;
        if (!run(kEightPoint, a.data(), b.data(), (uint32_t)data.size(), pose.rt.data(), &inl)) return std::nullopt;
        return std::make_pair(pose, std::move(inl));
    }
    std::optional<cv_core::CameraToCamera> model(const eight_point::EightPoint& e, const std::vector<cv_core::FeatureMatch>& data)
    {
        auto r = model_inliers(e, data);
        if (!r) return std::nullopt;
        return r->first;
    }
    // Consensus<NisterStewenius, FeatureMatch>::model_inliers (nister-stewenius/src/lib.rs:303-330 estimates): the builder's
    // hypothesis counts are five-match samples, each with up to ten essential matrices (include/akz.h RS_ESTIMATOR_FIVE_POINT)
    std::optional<std::pair<cv_core::CameraToCamera, std::vector<std::size_t>>> model_inliers(const nister_stewenius::NisterStewenius&,
                                                                                              const std::vector<cv_core::FeatureMatch>& data)
    {
        if (data.size() < nister_stewenius::NisterStewenius::MIN_SAMPLES) return std::nullopt;
        std::vector<double> a(3 * data.size()), b(3 * data.size());
        for (std::size_t i = 0; i < data.size(); ++i)
            for (int k = 0; k < 3; ++k) {
                a[3 * i + k] = data[i].a[k];
                b[3 * i + k] = data[i].b[k];
            }
        cv_core::CameraToCamera pose{};
        std::vector<std::size_t> inl;
        if (!run(kFivePoint, a.data(), b.data(), (uint32_t)data.size(), pose.rt.data(), &inl)) return std::nullopt;
        return std::make_pair(pose, std::move(inl));
    }
    std::optional<cv_core::CameraToCamera> model(const nister_stewenius::NisterStewenius& e, const std::vector<cv_core::FeatureMatch>& data)
    {
        auto r = model_inliers(e, data);
        if (!r) return std::nullopt;
        return r->first;
    }
    // Consensus<LambdaTwist, FeatureWorldMatch>::model_inliers (lambda-twist/src/lib.rs:330-347, cv-core/src/pose.rs:194-201)
    std::optional<std::pair<cv_core::WorldToCamera, std::vector<std::size_t>>> model_inliers(const lambda_twist::LambdaTwist&,
                                                                                             const std::vector<cv_core::FeatureWorldMatch>& data)
    {
        if (data.size() < lambda_twist::LambdaTwist::MIN_SAMPLES) return std::nullopt;
        std::vector<double> a(3 * data.size()), w(4 * data.size());
        for (std::size_t i = 0; i < data.size(); ++i) {
            for (int k = 0; k < 3; ++k) a[3 * i + k] = data[i].bearing[k];
            for (int k = 0; k < 4; ++k) w[4 * i + k] = data[i].world[k];
        }
        cv_core::WorldToCamera pose{};
        std::vector<std::size_t> inl;
        if (!run(kP3P, a.data(), w.data(), (uint32_t)data.size(), pose.rt.data(), &inl)) return std::nullopt;
        return std::make_pair(pose, std::move(inl));
    }

private:
    enum Estimator { kEightPoint, kP3P, kFivePoint };
    bool run(Estimator est, const double* a, const double* b, uint32_t n, double* pose, std::vector<std::size_t>* inl)
    {
        const bool p3p = est == kP3P;
        const uint32_t blocks = (n + p_.block_size - 1) / p_.block_size;
        // (a five-point sample takes ten hypothesis slots of the context)
        const uint32_t need_h = (p_.n_hypotheses + p_.estimations_per_block * blocks) * (est == kFivePoint ? 10u : 1u);
        rs_arrsac_params prm = p_;
        if (est == kFivePoint) prm.flags |= RS_ESTIMATOR_FIVE_POINT;
        if (!ctx_ || n > cap_m_ || need_h > cap_h_) {
            if (ctx_) rs_destroy(ctx_);
            ctx_ = nullptr;
            cap_m_ = n < 64 ? 64 : n;
            cap_h_ = need_h;
            akaze::require_abi();
            akaze::check(rs_create(device_, cap_m_, cap_h_, &ctx_), "rs_create");
        }
        std::vector<uint32_t> idx(n);
        uint32_t best = 0, ninl = 0;
        const int32_t st = p3p ? rs_p3p_arrsac(ctx_, a, b, n, nullptr, &prm, pose, &best, idx.data(), n, &ninl, nullptr)
                               : rs_essential_arrsac(ctx_, a, b, n, nullptr, &prm, pose, &best, idx.data(), n, &ninl, nullptr);
        akaze::check(st, p3p ? "rs_p3p_arrsac" : "rs_essential_arrsac");
        if (best == 0xFFFFFFFFu) return false;     // Consensus::model_inliers returned None
        inl->assign(idx.begin(), idx.begin() + ninl);
        return true;
    }
    rs_arrsac_params p_;
    int device_;
    rs_ctx* ctx_ = nullptr;
    uint32_t cap_m_ = 0, cap_h_ = 0;
};

}  // namespace arrsac

// cv_geom::triangulation::LinearEigenTriangulator (cv-geom/src/triangulation.rs:39-130) with the two traits it implements
// (cv-core/src/triangulation.rs:8-67) over rs_triangulate_observations: the points are computed on the device; std::nullopt
// where the reference returns None.  A point is the reference's Projective form {x, y, z, w}.
namespace cv_geom {
class LinearEigenTriangulator {
public:
    explicit LinearEigenTriangulator(int device = 0) : device_(device) { rs_triangulate_params_default(&p_); }
    LinearEigenTriangulator(const LinearEigenTriangulator& o) : p_(o.p_), device_(o.device_) {}
    LinearEigenTriangulator& operator=(const LinearEigenTriangulator&) = delete;
    ~LinearEigenTriangulator() { if (ctx_) rs_destroy(ctx_); }
    LinearEigenTriangulator epsilon(double e) const { LinearEigenTriangulator t(*this); t.p_.eps = e; return t; }
    LinearEigenTriangulator max_iterations(std::size_t n) const
    {
        LinearEigenTriangulator t(*this);
        t.p_.max_sweeps = n == 0 || n > 0x7FFFFFFFu ? 0x7FFFFFFFu : (uint32_t)n;     // (nalgebra: 0 = no limit)
        return t;
    }
    // TriangulatorObservations::triangulate_observations: (WorldToCamera, bearing) pairs -> WorldPoint
    std::optional<std::array<double, 4>> triangulate_observations(
        const std::vector<std::pair<cv_core::WorldToCamera, std::array<double, 3>>>& pairs)
    {
        std::vector<double> poses, bearings;
        for (const auto& pr : pairs) {
            poses.insert(poses.end(), pr.first.rt.begin(), pr.first.rt.end());
            bearings.insert(bearings.end(), pr.second.begin(), pr.second.end());
        }
        if (!ctx_) {
            akaze::require_abi();
            akaze::check(rs_create(device_, 8, 1, &ctx_), "rs_create");
        }
        std::array<double, 4> point{};
        uint8_t why = 0;
        akaze::check(rs_triangulate_observations(ctx_, poses.data(), bearings.data(), (uint32_t)pairs.size(), &p_, point.data(), &why),
                     "rs_triangulate_observations");
        last_reason_ = why;
        if (why != RS_TRI_OK) return std::nullopt;
        return point;
    }
    // TriangulatorObservations::triangulate_observations_to_camera: the first camera is the world (identity)
    std::optional<std::array<double, 4>> triangulate_observations_to_camera(
        const std::array<double, 3>& center_bearing, const std::vector<std::pair<cv_core::CameraToCamera, std::array<double, 3>>>& pairs)
    {
        std::vector<std::pair<cv_core::WorldToCamera, std::array<double, 3>>> all;
        all.push_back({cv_core::WorldToCamera{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}}, center_bearing});
        for (const auto& pr : pairs) all.push_back({cv_core::WorldToCamera{pr.first.rt}, pr.second});
        return triangulate_observations(all);
    }
    // TriangulatorRelative::triangulate_relative
    std::optional<std::array<double, 4>> triangulate_relative(const cv_core::CameraToCamera& pose, const std::array<double, 3>& a,
                                                              const std::array<double, 3>& b)
    {
        return triangulate_observations_to_camera(a, {{pose, b}});
    }
    uint8_t last_reason() const { return last_reason_; }   // RS_TRI_* of the last call

private:
    rs_triangulate_params p_;
    int device_;
    rs_ctx* ctx_ = nullptr;
    uint8_t last_reason_ = 0;
};
}  // namespace cv_geom

// cv-sfm's three-view bootstrap (VSlam::init_reconstruction from its common matches on, cv-sfm/src/lib.rs:1002-1300) over
// rs_three_view_init_batch_device: every argument named d_* is device memory the caller owns (the layouts are include/akz.h's),
// the call enqueues on stream() and returns.  The join of the two pair lists and the shuffle are ReconstructionStart's (below).
namespace cv_sfm {
class ThreeViewInit {
public:
    // room for `max_scenes` triples per call
    explicit ThreeViewInit(uint32_t max_scenes = 1, int device = 0)
    {
        akaze::require_abi();
        rs_three_view_params_default(&p_);
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
        const int32_t st = rs_batch_reserve(ctx_, max_scenes);
        if (st != AKZ_OK) {
            rs_destroy(ctx_);
            akaze::check(st, "rs_batch_reserve");
        }
    }
    ~ThreeViewInit() { if (ctx_) rs_destroy(ctx_); }
    ThreeViewInit(const ThreeViewInit&) = delete;
    ThreeViewInit& operator=(const ThreeViewInit&) = delete;
    rs_three_view_params& params() { return p_; }   // the reference's defaults (cv-sfm/src/settings.rs:320-427) to begin with
    const rs_three_view_params& params() const { return p_; }
    // one block index per scene in ic / i_first / i_second; outputs as include/akz.h documents them
    void init_batch_device(const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const std::vector<uint32_t>& ic,
                           const std::vector<uint32_t>& i_first, const std::vector<uint32_t>& i_second, const rs_camera& cam,
                           const void* d_pose_first, const void* d_pose_second, const void* d_triples, const void* d_ntriples,
                           const void* d_first_only, const void* d_nfirst, const void* d_second_only, const void* d_nsecond,
                           void* d_pose_out, void* d_verdict, void* d_combined, void* d_first_ok, void* d_second_ok, void* d_stats,
                           void* stream_to_wait = nullptr)
    {
        if (i_first.size() != ic.size() || i_second.size() != ic.size()) throw std::invalid_argument("one centre, first and second block per scene");
        akaze::check(rs_three_view_init_batch_device(ctx_, d_kps, cap_per_img, n_blocks, ic.data(), i_first.data(), i_second.data(), &cam,
                                                     d_pose_first, d_pose_second, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only,
                                                     d_nsecond, (uint32_t)ic.size(), &p_, d_pose_out, d_verdict, d_combined, d_first_ok,
                                                     d_second_ok, d_stats, stream_to_wait),
                     "rs_three_view_init_batch_device");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_three_view_params p_;
    rs_ctx* ctx_ = nullptr;
};

// cv-sfm's three-view constraints of the pose graph (VSlam::optimize_three_view behind its shuffle and sort,
// cv-sfm/src/lib.rs:1939-2062) over rs_three_view_constraint_batch_device, one wavefront per constraint: every argument named
// d_* is device memory the caller owns (the layouts are include/akz.h's), the call enqueues on stream() and returns.  The
// shuffle and the unstable sort by observation count stay with the caller.
class ThreeViewConstraints {
public:
    explicit ThreeViewConstraints(int device = 0)
    {
        akaze::require_abi();
        rs_three_view_constraint_params_default(&p_);
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~ThreeViewConstraints() { if (ctx_) rs_destroy(ctx_); }
    ThreeViewConstraints(const ThreeViewConstraints&) = delete;
    ThreeViewConstraints& operator=(const ThreeViewConstraints&) = delete;
    rs_three_view_constraint_params& params() { return p_; }   // the reference's defaults (cv-sfm/src/settings.rs:332-338, 465-483)
    const rs_three_view_constraint_params& params() const { return p_; }
    void batch_device(const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses, const rs_camera& cam,
                      const void* d_views, const void* d_lm_start, const void* d_lm, uint32_t n_lm, uint32_t n_constraints,
                      void* d_pose_out, void* d_verdict, void* d_stats, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_three_view_constraint_batch_device(ctx_, d_kps, cap_per_img, n_blocks, d_poses, &cam, d_views, d_lm_start, d_lm, n_lm,
                                                           n_constraints, &p_, d_pose_out, d_verdict, d_stats, stream_to_wait),
                     "rs_three_view_constraint_batch_device");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_three_view_constraint_params p_;
    rs_ctx* ctx_ = nullptr;
};

// cv-sfm's relaxation of the pose graph under its three-view constraints (VSlam::apply_constraints,
// cv-sfm/src/lib.rs:2358-2375) over rs_pose_graph_edges_device and rs_pose_graph_relax_batch_device, one wavefront per view
// and round: every argument named d_* is device memory the caller owns (the layouts are include/akz.h's), the calls enqueue on
// stream() and return.  flatten() builds the rows on the host in the documented admissible order: constraint index
// ascending, slot order within a constraint.
class PoseGraph {
public:
    explicit PoseGraph(int device = 0)
    {
        akaze::require_abi();
        rs_pose_graph_params_default(&p_);
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~PoseGraph() { if (ctx_) rs_destroy(ctx_); }
    PoseGraph(const PoseGraph&) = delete;
    PoseGraph& operator=(const PoseGraph&) = delete;
    rs_pose_graph_params& params() { return p_; }   // the reference's defaults (cv-sfm/src/settings.rs:461-463, 477-479)
    const rs_pose_graph_params& params() const { return p_; }
    // views [n][3] -> row_start [n_views + 1], row_edges [6 n] (edge id 6 * constraint + slot); false: a view >= n_views
    static bool flatten(const std::vector<uint32_t>& views, uint32_t n_views, std::vector<uint32_t>& row_start, std::vector<uint32_t>& row_edges)
    {
        static const uint32_t target[6] = {0, 0, 1, 1, 2, 2};
        const size_t n = views.size() / 3;
        row_start.assign((size_t)n_views + 1, 0u);
        for (size_t c = 0; c < n; ++c)
            for (int s = 0; s < 6; ++s) {
                if (views[3 * c + target[s]] >= n_views) return false;
                ++row_start[(size_t)views[3 * c + target[s]] + 1];
            }
        for (uint32_t v = 0; v < n_views; ++v) row_start[v + 1] += row_start[v];
        row_edges.assign(6 * n, 0u);
        std::vector<uint32_t> at(row_start.begin(), row_start.end() - 1);
        for (size_t c = 0; c < n; ++c)
            for (int s = 0; s < 6; ++s) row_edges[at[views[3 * c + target[s]]]++] = (uint32_t)(6 * c + s);
        return true;
    }
    void edges_device(const void* d_views, const void* d_constraint_poses, const void* d_constraint_verdict, uint32_t n_constraints,
                      void* d_edges, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_pose_graph_edges_device(ctx_, d_views, d_constraint_poses, d_constraint_verdict, n_constraints, d_edges, stream_to_wait),
                     "rs_pose_graph_edges_device");
    }
    void relax_batch_device(void* d_poses, uint32_t n_views, const void* d_graph_start, uint32_t n_graphs, const void* d_row_start,
                            const void* d_row_edges, uint32_t n_rows, const void* d_views, const void* d_constraint_verdict,
                            const void* d_edges, uint32_t n_constraints, void* d_graph_verdict, void* d_view_state, void* d_stats,
                            void* stream_to_wait = nullptr)
    {
        akaze::check(rs_pose_graph_relax_batch_device(ctx_, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows, d_views,
                                                      d_constraint_verdict, d_edges, n_constraints, &p_, d_graph_verdict, d_view_state, d_stats,
                                                      stream_to_wait),
                     "rs_pose_graph_relax_batch_device");
    }
    // flatten() on the device (rs_pose_graph_rows_device): d_row_start [n_views + 1], d_row_edges [6 n], d_flags [1] (1: a triple
    // named a view >= n_views and is in no row)
    void rows(const void* d_views, uint32_t n_constraints, uint32_t n_views, void* d_row_start, void* d_row_edges, void* d_flags,
              void* stream_to_wait = nullptr)
    {
        akaze::check(rs_pose_graph_rows_device(ctx_, d_views, n_constraints, n_views, d_row_start, d_row_edges, d_flags, stream_to_wait),
                     "rs_pose_graph_rows_device");
    }
    // parity tap: graphs of more than `views` views (at most RS_PG_RESIDENT_VIEWS) take the swept form from now on
    void resident_views(uint32_t views) { akaze::check(rs_pose_graph_debug_resident_views(ctx_, views), "rs_pose_graph_debug_resident_views"); }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }
    rs_ctx* context() { return ctx_; }

private:
    rs_pose_graph_params p_;
    rs_ctx* ctx_ = nullptr;
};

// cv-sfm's filter of a reconstruction's observations behind a relaxation (VSlam::filter_non_robust_observations,
// cv-sfm/src/lib.rs:2657-2757) over rs_filter_observations_device: one lane per landmark decides, an exclusive scan over the
// observations compacts the table.  Every argument named d_* is device memory the caller owns (the layouts are
// include/akz.h's); the calls enqueue on stream() and return.
class ObservationFilter {
public:
    explicit ObservationFilter(int device = 0)
    {
        akaze::require_abi();
        rs_observation_filter_params_default(&p_);
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~ObservationFilter() { if (ctx_) rs_destroy(ctx_); }
    ObservationFilter(const ObservationFilter&) = delete;
    ObservationFilter& operator=(const ObservationFilter&) = delete;
    rs_observation_filter_params& params() { return p_; }   // the reference's defaults (cv-sfm/src/settings.rs:324-350, 429-431)
    const rs_observation_filter_params& params() const { return p_; }
    void filter_device(const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses, const rs_camera& cam,
                       const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, const void* d_recon_start,
                       const void* d_view_start, uint32_t n_recons, const void* d_skip, void* d_keep, void* d_lm_state, void* d_tri_reason,
                       void* d_robust, void* d_obs_start_out, void* d_obs_out, void* d_split_out, void* d_counts, void* d_recon_verdict,
                       void* d_stats, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_filter_observations_device(ctx_, d_kps, cap_per_img, n_blocks, d_poses, &cam, d_obs_start, d_obs, n_obs, n_landmarks,
                                                   d_recon_start, d_view_start, n_recons, d_skip, &p_, d_keep, d_lm_state, d_tri_reason, d_robust,
                                                   d_obs_start_out, d_obs_out, d_split_out, d_counts, d_recon_verdict, d_stats, stream_to_wait),
                     "rs_filter_observations_device");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }
    rs_ctx* context() { return ctx_; }

private:
    rs_observation_filter_params p_;
    rs_ctx* ctx_ = nullptr;
};

// VSlam::optimize_reconstruction (cv-sfm/src/lib.rs:2343-2355) over rs_optimize_reconstruction_batch_device, on the filter's
// context: filter.params().reconstruction_optimization_iterations rounds of the relaxation (under `pg`) and the filter, then
// the world table of the final lists into d_world (may be null).  Where a reconstruction stopped is d_verdict's word (RS_OR_*).
inline void optimize_reconstruction(ObservationFilter& filter, const rs_pose_graph_params& pg, void* d_poses, uint32_t n_views,
                                    const void* d_graph_start, uint32_t n_graphs, const void* d_row_start, const void* d_row_edges, uint32_t n_rows,
                                    const void* d_views, const void* d_constraint_verdict, const void* d_edges, uint32_t n_constraints,
                                    const void* d_kps, uint32_t cap_per_img, const rs_camera& cam, const void* d_obs_start, const void* d_obs,
                                    uint32_t n_obs, uint32_t n_landmarks, const void* d_recon_start, void* d_verdict, void* d_graph_verdict,
                                    void* d_view_state, void* d_pg_stats, void* d_keep, void* d_lm_state, void* d_tri_reason, void* d_robust,
                                    void* d_obs_start_out, void* d_obs_out, void* d_split_out, void* d_counts, void* d_recon_verdict,
                                    void* d_of_stats, void* d_world = nullptr, void* d_world_reason = nullptr, void* stream_to_wait = nullptr)
{
    akaze::check(rs_optimize_reconstruction_batch_device(filter.context(), d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows,
                                                         d_views, d_constraint_verdict, d_edges, n_constraints, &pg, d_kps, cap_per_img, &cam,
                                                         d_obs_start, d_obs, n_obs, n_landmarks, d_recon_start, &filter.params(), d_verdict,
                                                         d_graph_verdict, d_view_state, d_pg_stats, d_keep, d_lm_state, d_tri_reason, d_robust,
                                                         d_obs_start_out, d_obs_out, d_split_out, d_counts, d_recon_verdict, d_of_stats, d_world,
                                                         d_world_reason, stream_to_wait),
                 "rs_optimize_reconstruction_batch_device");
}

// cv-sfm's covisibility search in front of its three-view constraints (VSlam::generate_view_constraints, cv-sfm/src/lib.rs:
// 2438-2516) and the verdict of record_view_constraints (lib.rs:2092-2109) over rs_covisibility_candidates_device and
// rs_covisibility_record_device.  It works on a context it does not own (`ctx`: the one the constraint stage and the pose
// graph run on, so that the chain queues on one stream).  Every argument named d_* is device memory the caller owns (the
// layouts are include/akz.h's); the calls enqueue and return.
class ViewConstraints {
public:
    enum Verdict : uint32_t { Ok = RS_CV_OK, FewConstraints = RS_CV_FEW_CONSTRAINTS, BadIndex = RS_CV_BAD_INDEX, NoGraph = RS_CV_NO_GRAPH };
    explicit ViewConstraints(rs_ctx* ctx) : ctx_(ctx)
    {
        akaze::require_abi();
        rs_covisibility_params_default(&p_);
    }
    rs_covisibility_params& params() { return p_; }   // the reference's defaults (cv-sfm/src/settings.rs:453-475)
    const rs_covisibility_params& params() const { return p_; }
    uint32_t limit() const { return p_.candidate_limit ? p_.candidate_limit : p_.optimization_maximum_three_view_constraints; }   // slots per target
    void candidates_device(const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t cap_per_img,
                           uint32_t n_blocks, const void* d_reason, const void* d_targets, uint32_t n_targets, void* d_views, void* d_lm_start,
                           void* d_lm, void* d_slot_count, void* d_target_verdict, void* d_stats, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_covisibility_candidates_device(ctx_, d_obs_start, d_obs, n_obs, n_landmarks, cap_per_img, n_blocks, d_reason, d_targets,
                                                       n_targets, &p_, d_views, d_lm_start, d_lm, d_slot_count, d_target_verdict, d_stats,
                                                       stream_to_wait),
                     "rs_covisibility_candidates_device");
    }
    void record_device(const void* d_constraint_verdict, const void* d_targets, uint32_t n_targets, const void* d_graph_start, uint32_t n_graphs,
                       void* d_recorded, void* d_target_verdict, void* d_stats, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_covisibility_record_device(ctx_, d_constraint_verdict, d_targets, n_targets, d_graph_start, n_graphs, &p_, d_recorded,
                                                   d_target_verdict, d_stats, stream_to_wait),
                     "rs_covisibility_record_device");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_covisibility_params p_;
    rs_ctx* ctx_ = nullptr;
};

// What cv-sfm's register_frame_subset does behind its consensus (cv-sfm/src/lib.rs:1625-1775) over
// rs_refine_poses_batch_device: the single-view L2 optimiser and the consistency filter, one persistent workgroup per new
// frame.  It works on the context of the consensus that registered the frames (`ctx`, not owned: the call queues behind
// rs_p3p_arrsac_batch_device on that context's stream, no host step).  Every argument named d_* is device memory the caller
// owns (the layouts are include/akz.h's); the call enqueues and returns.
class SingleViewRefiner {
public:
    enum Verdict : uint32_t { Ok = RS_SV_OK, NoModel = RS_SV_NO_MODEL, FewLandmarks = RS_SV_FEW_LANDMARKS, LostHalf = RS_SV_LOST_HALF,
                              FewRobust = RS_SV_FEW_ROBUST, BadIndex = RS_SV_BAD_INDEX };
    explicit SingleViewRefiner(rs_ctx* ctx) : ctx_(ctx)
    {
        akaze::require_abi();
        rs_single_view_params_default(&p_);
    }
    rs_single_view_params& params() { return p_; }   // the reference's defaults (cv-sfm/src/settings.rs:324-383)
    const rs_single_view_params& params() const { return p_; }
    void refine_batch_device(const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses, const rs_camera& cam,
                             const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, const void* d_world,
                             uint32_t n_world, const std::vector<uint32_t>& ik, const void* d_matches, const void* d_nmatches, const void* d_best,
                             const void* d_pose, const void* d_best_id, const void* d_inliers, const void* d_n_inliers, void* d_pose_out,
                             void* d_verdict, void* d_final, void* d_n_final, void* d_stats, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_refine_poses_batch_device(ctx_, d_kps, cap_per_img, n_blocks, d_poses, &cam, d_obs_start, d_obs, n_obs, n_landmarks, d_world,
                                                  n_world, ik.data(), d_matches, d_nmatches, d_best, d_pose, d_best_id, d_inliers, d_n_inliers,
                                                  (uint32_t)ik.size(), &p_, d_pose_out, d_verdict, d_final, d_n_final, d_stats, stream_to_wait),
                     "rs_refine_poses_batch_device");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_single_view_params p_;
    rs_ctx* ctx_ = nullptr;
};

// cv-sfm's landmark bookkeeping around the registration of a micro-batch over rs_landmarks_sharing_view_device and
// rs_add_views_device: the graph test behind a merge candidate (VSlam::are_landmarks_sharing_view, cv-sfm/src/lib.rs:1435-1449)
// and VSlamData::add_view with merge_landmarks (lib.rs:432-483, 699-721) for the accepted frames, out of place.  It works on the
// context of the consensus that registered the frames (`ctx`, not owned: the calls queue behind the refinement on that
// context's stream, no host step) or, built from a device number, on a small context of its own.  Every argument named d_* is
// device memory the caller owns (the layouts are include/akz.h's); the calls enqueue and return.
class LandmarkBook {
public:
    enum Verdict : uint32_t { Ok = RS_AV_OK, NotAccepted = RS_AV_NOT_ACCEPTED, BadIndex = RS_AV_BAD_INDEX, BadTable = RS_AV_BAD_TABLE };
    explicit LandmarkBook(rs_ctx* ctx) : ctx_(ctx) { akaze::require_abi(); }
    explicit LandmarkBook(int device = 0) : owned_(true)
    {
        akaze::require_abi();
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~LandmarkBook() { if (owned_ && ctx_) rs_destroy(ctx_); }
    LandmarkBook(const LandmarkBook&) = delete;
    LandmarkBook& operator=(const LandmarkBook&) = delete;
    void sharing_view(const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, const void* d_best, const void* d_decision,
                      uint32_t cap_per_img, uint32_t n_frames, void* d_merge_ok, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_landmarks_sharing_view_device(ctx_, d_obs_start, d_obs, n_obs, n_landmarks, d_best, d_decision, cap_per_img, n_frames,
                                                      d_merge_ok, stream_to_wait),
                     "rs_landmarks_sharing_view_device");
    }
    void add_views(const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t n_world, const void* d_split,
                   const void* d_split_count, uint32_t split_room, uint32_t cap_per_img, uint32_t n_blocks, const std::vector<uint32_t>& ik,
                   const void* d_counts, const void* d_matches, const void* d_nmatches, const void* d_final, const void* d_verdict,
                   const void* d_pose_out, const void* d_best, const void* d_skip, uint32_t obs_room, uint32_t lm_room, void* d_poses,
                   void* d_obs_start_out, void* d_obs_out, void* d_counts_out, void* d_landmarks_out, void* d_obs_counts_out,
                   void* d_frame_verdict, void* d_stats, void* d_call_verdict, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_add_views_device(ctx_, d_obs_start, d_obs, n_obs, n_landmarks, n_world, d_split, d_split_count, split_room, cap_per_img,
                                         n_blocks, ik.data(), (uint32_t)ik.size(), d_counts, d_matches, d_nmatches, d_final, d_verdict, d_pose_out,
                                         d_best, d_skip, obs_room, lm_room, d_poses, d_obs_start_out, d_obs_out, d_counts_out, d_landmarks_out,
                                         d_obs_counts_out, d_frame_verdict, d_stats, d_call_verdict, stream_to_wait),
                     "rs_add_views_device");
    }
    // the least rooms add_views accepts
    static uint64_t room(uint32_t n, uint32_t split_room, uint32_t n_frames, uint32_t cap_per_img)
    {
        return (uint64_t)n + split_room + (uint64_t)n_frames * cap_per_img;
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_ctx* ctx_ = nullptr;
    bool owned_ = false;
};

// A reconstruction repacked over rs_repack_table_device, rs_gather_blocks_device and rs_repack_constraints_device:
// VSlamData::remove_view (cv-sfm/src/lib.rs:517-546) for every view a block map removes at once, the table compacted, rows and
// blocks renumbered, the per-block pools and the constraints moved along.  A repacked table always fits
// room(n_blocks_out, cap_per_img) rows and observations.  Contexts and arguments as LandmarkBook's; the calls enqueue and return.
class TableRepack {
public:
    enum Verdict : uint32_t { Ok = RS_RP_OK, BadTable = RS_RP_BAD_TABLE, BadIndex = RS_RP_BAD_INDEX, BadMap = RS_RP_BAD_MAP, NoRoom = RS_RP_NO_ROOM };
    static constexpr uint32_t kRemoved = 0xFFFFFFFFu;       // a block map's entry for a removed view
    explicit TableRepack(rs_ctx* ctx) : ctx_(ctx) { akaze::require_abi(); }
    explicit TableRepack(int device = 0) : owned_(true)
    {
        akaze::require_abi();
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~TableRepack() { if (owned_ && ctx_) rs_destroy(ctx_); }
    TableRepack(const TableRepack&) = delete;
    TableRepack& operator=(const TableRepack&) = delete;
    void table(const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t cap_per_img, uint32_t n_blocks,
               const void* d_block_map, uint32_t n_blocks_out, const void* d_recon_start, uint32_t n_recons, uint32_t obs_room, uint32_t lm_room,
               void* d_obs_start_out, void* d_obs_out, void* d_obs_counts_out, void* d_landmarks_out, void* d_key_out, void* d_recon_start_out,
               void* d_counts_out, void* d_call_verdict, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_repack_table_device(ctx_, d_obs_start, d_obs, n_obs, n_landmarks, cap_per_img, n_blocks, d_block_map, n_blocks_out,
                                            d_recon_start, n_recons, obs_room, lm_room, d_obs_start_out, d_obs_out, d_obs_counts_out,
                                            d_landmarks_out, d_key_out, d_recon_start_out, d_counts_out, d_call_verdict, stream_to_wait),
                     "rs_repack_table_device");
    }
    void gather(const void* d_src, void* d_dst, uint32_t row_bytes, uint32_t n_blocks, const void* d_block_map, uint32_t n_blocks_out,
                void* d_verdict, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_gather_blocks_device(ctx_, d_src, d_dst, row_bytes, n_blocks, d_block_map, n_blocks_out, d_verdict, stream_to_wait),
                     "rs_gather_blocks_device");
    }
    void constraints(const void* d_views, const void* d_constraint_poses, const void* d_constraint_verdict, uint32_t n_constraints,
                     const void* d_block_map, uint32_t n_blocks, uint32_t n_blocks_out, const void* d_start, uint32_t n_ranges, void* d_views_out,
                     void* d_constraint_poses_out, void* d_constraint_verdict_out, void* d_count, void* d_start_out,
                     void* stream_to_wait = nullptr)
    {
        akaze::check(rs_repack_constraints_device(ctx_, d_views, d_constraint_poses, d_constraint_verdict, n_constraints, d_block_map, n_blocks,
                                                  n_blocks_out, d_start, n_ranges, d_views_out, d_constraint_poses_out, d_constraint_verdict_out,
                                                  d_count, d_start_out, stream_to_wait),
                     "rs_repack_constraints_device");
    }
    // the rooms no valid repacked table outgrows
    static uint64_t room(uint32_t n_blocks_out, uint32_t cap_per_img) { return (uint64_t)n_blocks_out * cap_per_img; }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_ctx* ctx_ = nullptr;
    bool owned_ = false;
};

// cv-sfm's loop closure between two reconstructions and its normalisation over rs_merge_map_device,
// rs_incorporate_reconstruction_device and rs_normalize_reconstruction_device: the landmark map of the bridging frame
// (VSlam::try_merge_reconstructions, cv-sfm/src/lib.rs:2159-2170), incorporate_reconstruction (lib.rs:1817-1887), out of place,
// and normalize_reconstruction (lib.rs:2241-2283).  It works on the context of the consensus that registered the bridging frame
// (`ctx`, not owned) or, built from a device number, on a small context of its own.  Every argument named d_* is device memory
// the caller owns (the layouts are include/akz.h's); the calls enqueue and return.
class ReconstructionMerge {
public:
    enum Verdict : uint32_t { Ok = RS_IR_OK, BadTable = RS_IR_BAD_TABLE, BadIndex = RS_IR_BAD_INDEX, SharedBlock = RS_IR_SHARED_BLOCK };
    enum NormalizeVerdict : uint32_t { Normalized = RS_NR_OK, NotNormal = RS_NR_NOT_NORMAL, NormalizeBadIndex = RS_NR_BAD_INDEX };
    explicit ReconstructionMerge(rs_ctx* ctx) : ctx_(ctx) { akaze::require_abi(); }
    explicit ReconstructionMerge(int device = 0) : owned_(true)
    {
        akaze::require_abi();
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~ReconstructionMerge() { if (owned_ && ctx_) rs_destroy(ctx_); }
    ReconstructionMerge(const ReconstructionMerge&) = delete;
    ReconstructionMerge& operator=(const ReconstructionMerge&) = delete;
    void merge_map(const void* d_matches, const void* d_nmatches, const void* d_final, const void* d_best, uint32_t n_world,
                   uint32_t n_dst_landmarks, uint32_t cap_per_img, uint32_t slot, const void* d_counts, const void* d_src_landmarks,
                   uint32_t n_blocks, uint32_t bridge_block, void* d_map, void* d_map_count, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_merge_map_device(ctx_, d_matches, d_nmatches, d_final, d_best, n_world, n_dst_landmarks, cap_per_img, slot, d_counts,
                                         d_src_landmarks, n_blocks, bridge_block, d_map, d_map_count, stream_to_wait),
                     "rs_merge_map_device");
    }
    void incorporate(const void* d_dst_start, const void* d_dst_obs, uint32_t n_dst_obs, uint32_t n_dst_landmarks, const void* d_src_start,
                     const void* d_src_obs, uint32_t n_src_obs, uint32_t n_src_landmarks, const void* d_map, const void* d_map_count,
                     uint32_t map_room, uint32_t cap_per_img, uint32_t n_blocks, const std::vector<uint32_t>& src_blocks, uint32_t bridge_block,
                     const void* d_src_pose, const void* d_skip, uint32_t obs_room, uint32_t lm_room, void* d_poses, void* d_obs_start_out,
                     void* d_obs_out, void* d_counts_out, void* d_landmarks_out, void* d_obs_counts_out, void* d_src_key_out,
                     void* d_call_verdict, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_incorporate_reconstruction_device(ctx_, d_dst_start, d_dst_obs, n_dst_obs, n_dst_landmarks, d_src_start, d_src_obs,
                                                          n_src_obs, n_src_landmarks, d_map, d_map_count, map_room, cap_per_img, n_blocks,
                                                          src_blocks.data(), (uint32_t)src_blocks.size(), bridge_block, d_src_pose, d_skip,
                                                          obs_room, lm_room, d_poses, d_obs_start_out, d_obs_out, d_counts_out, d_landmarks_out,
                                                          d_obs_counts_out, d_src_key_out, d_call_verdict, stream_to_wait),
                     "rs_incorporate_reconstruction_device");
    }
    void normalize(const std::vector<uint32_t>& view_blocks, const void* d_counts, const void* d_landmarks, uint32_t cap_per_img,
                   uint32_t n_blocks, const void* d_world, uint32_t n_world, void* d_poses, void* d_constraint_poses, uint32_t n_constraints,
                   void* d_stats, void* d_verdict, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_normalize_reconstruction_device(ctx_, view_blocks.data(), (uint32_t)view_blocks.size(), d_counts, d_landmarks,
                                                        cap_per_img, n_blocks, d_world, n_world, d_poses, d_constraint_poses, n_constraints,
                                                        d_stats, d_verdict, stream_to_wait),
                     "rs_normalize_reconstruction_device");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_ctx* ctx_ = nullptr;
    bool owned_ = false;
};

// VSlam::export_reconstruction (cv-sfm/src/lib.rs:2285-2340) with export.rs over rs_export_reconstruction_device and
// rs_write_ply: the coloured point cloud and the cameras' frusta as the vertex arrays of the .ply file, made on the device, and
// the file's text, written by the host.  It works on the context of the consensus whose stream made the world table (`ctx`,
// not owned) or, built from a device number, on a small context of its own.  Every argument named d_* is device memory the
// caller owns (the layouts are include/akz.h's); export_device enqueues and returns.
class ReconstructionExport {
public:
    enum Verdict : uint32_t { Ok = RS_EX_OK, Overflow = RS_EX_OVERFLOW, BadTable = RS_EX_BAD_TABLE };
    explicit ReconstructionExport(rs_ctx* ctx) : ctx_(ctx) { akaze::require_abi(); }
    explicit ReconstructionExport(int device = 0) : owned_(true)
    {
        akaze::require_abi();
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~ReconstructionExport() { if (owned_ && ctx_) rs_destroy(ctx_); }
    ReconstructionExport(const ReconstructionExport&) = delete;
    ReconstructionExport& operator=(const ReconstructionExport&) = delete;
    void export_device(const void* d_world, uint32_t n_world, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks,
                       const void* d_colors, const std::vector<uint32_t>& view_blocks, const void* d_counts, const void* d_landmarks,
                       uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses, uint32_t room, void* d_xyz, void* d_rgb, void* d_key,
                       void* d_cameras, void* d_counts_out, void* d_verdict, void* stream_to_wait = nullptr)
    {
        akaze::check(rs_export_reconstruction_device(ctx_, d_world, n_world, d_obs_start, d_obs, n_obs, n_landmarks, d_colors, view_blocks.data(),
                                                     (uint32_t)view_blocks.size(), d_counts, d_landmarks, cap_per_img, n_blocks, d_poses, room,
                                                     d_xyz, d_rgb, d_key, d_cameras, d_counts_out, d_verdict, stream_to_wait),
                     "rs_export_reconstruction_device");
    }
    // host arrays xyz [n][3], rgb [n][3] whose first 5 * n_cameras rows are the cameras' vertices -> the file export.rs writes
    static void write_ply(const std::string& path, const std::vector<double>& xyz, const std::vector<uint8_t>& rgb, uint32_t n_cameras,
                          bool camera_faces)
    {
        if (xyz.size() != rgb.size() || xyz.size() % 3) throw std::invalid_argument("one colour per vertex");
        akaze::check(rs_write_ply(path.c_str(), xyz.data(), rgb.data(), (uint32_t)(xyz.size() / 3), n_cameras, camera_faces ? 1 : 0),
                     "rs_write_ply");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_ctx* ctx_ = nullptr;
    bool owned_ = false;
};

// The two integer steps of cv-sfm's try_init around the three-view bootstrap, over rs_join_pairs_batch_device (the join and the
// shuffle of VSlam::init_reconstruction, cv-sfm/src/lib.rs:992-999, 1190-1191, 1216, 1234) and
// rs_add_reconstruction_batch_device (VSlamData::add_reconstruction, lib.rs:377-427): the lists the bootstrap reads and the first
// generation of the landmark table, made on the device.  It works on the context of the consensus whose stream made the inlier
// lists (`ctx`, not owned) or, built from a device number, on a small context of its own.  Every argument named d_* is device
// memory the caller owns (the layouts are include/akz.h's); both calls enqueue and return.
class ReconstructionStart {
public:
    enum JoinVerdict : uint32_t { JoinOk = RS_JP_OK, NoModel = RS_JP_NO_MODEL, FewInliers = RS_JP_FEW_INLIERS, JoinBadIndex = RS_JP_BAD_INDEX };
    enum Verdict : uint32_t { Ok = RS_AR_OK, NotAccepted = RS_AR_NOT_ACCEPTED, BadIndex = RS_AR_BAD_INDEX, Taken = RS_AR_TAKEN, BadTable = RS_AR_BAD_TABLE };
    explicit ReconstructionStart(rs_ctx* ctx) : ctx_(ctx) { akaze::require_abi(); }
    explicit ReconstructionStart(int device = 0) : owned_(true)
    {
        akaze::require_abi();
        akaze::check(rs_create(device, 8, 1, &ctx_), "rs_create");
    }
    ~ReconstructionStart() { if (owned_ && ctx_) rs_destroy(ctx_); }
    ReconstructionStart(const ReconstructionStart&) = delete;
    ReconstructionStart& operator=(const ReconstructionStart&) = delete;
    void join_pairs_device(const void* d_pairs, const void* d_npairs, const void* d_inliers, const void* d_n_inliers, const void* d_best_id,
                           const void* d_pose, uint32_t n_slots, uint32_t cap_per_img, const std::vector<uint32_t>& slot_first,
                           const std::vector<uint32_t>& slot_second, uint32_t two_view_minimum_robust_matches, uint32_t flags, uint64_t seed,
                           void* d_triples, void* d_ntriples, void* d_first_only, void* d_nfirst, void* d_second_only, void* d_nsecond,
                           void* d_pose_first, void* d_pose_second, void* d_verdict, void* stream_to_wait = nullptr)
    {
        if (slot_second.size() != slot_first.size()) throw std::invalid_argument("one first and one second slot per scene");
        akaze::check(rs_join_pairs_batch_device(ctx_, d_pairs, d_npairs, d_inliers, d_n_inliers, d_best_id, d_pose, n_slots, cap_per_img,
                                                slot_first.data(), slot_second.data(), (uint32_t)slot_first.size(),
                                                two_view_minimum_robust_matches, flags, seed, d_triples, d_ntriples, d_first_only, d_nfirst,
                                                d_second_only, d_nsecond, d_pose_first, d_pose_second, d_verdict, stream_to_wait),
                     "rs_join_pairs_batch_device");
    }
    void add_reconstruction_device(const void* d_triples, const void* d_ntriples, const void* d_first_only, const void* d_nfirst,
                                   const void* d_second_only, const void* d_nsecond, const void* d_combined, const void* d_first_ok,
                                   const void* d_second_ok, const void* d_pose_out, const void* d_verdict, const std::vector<uint32_t>& ic,
                                   const std::vector<uint32_t>& i_first, const std::vector<uint32_t>& i_second, const void* d_kps,
                                   const void* d_counts, uint32_t n_src_blocks, uint32_t cap_per_img, const void* d_skip, const void* d_obs_start,
                                   const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, const void* d_recon_start, const void* d_view_start,
                                   uint32_t n_recons, void* d_kps_dst, void* d_counts_dst, void* d_poses, uint32_t n_blocks, uint32_t view_base,
                                   uint32_t obs_room, uint32_t lm_room, void* d_obs_start_out, void* d_obs_out, void* d_obs_counts_out,
                                   void* d_counts_out, void* d_landmarks_out, void* d_recon_start_out, void* d_view_start_out, void* d_views_out,
                                   void* d_constraint_poses_out, void* d_constraint_verdict_out, void* d_frame_verdict, void* d_stats,
                                   void* d_call_verdict, void* stream_to_wait = nullptr)
    {
        if (i_first.size() != ic.size() || i_second.size() != ic.size()) throw std::invalid_argument("one centre, first and second block per scene");
        akaze::check(rs_add_reconstruction_batch_device(ctx_, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond, d_combined,
                                                        d_first_ok, d_second_ok, d_pose_out, d_verdict, ic.data(), i_first.data(), i_second.data(),
                                                        (uint32_t)ic.size(), d_kps, d_counts, n_src_blocks, cap_per_img, d_skip, d_obs_start, d_obs,
                                                        n_obs, n_landmarks, d_recon_start, d_view_start, n_recons, d_kps_dst, d_counts_dst, d_poses,
                                                        n_blocks, view_base, obs_room, lm_room, d_obs_start_out, d_obs_out, d_obs_counts_out,
                                                        d_counts_out, d_landmarks_out, d_recon_start_out, d_view_start_out, d_views_out,
                                                        d_constraint_poses_out, d_constraint_verdict_out, d_frame_verdict, d_stats, d_call_verdict,
                                                        stream_to_wait),
                     "rs_add_reconstruction_batch_device");
    }
    void sync() { akaze::check(rs_sync(ctx_), "rs_sync"); }
    void* stream() { return rs_stream(ctx_); }

private:
    rs_ctx* ctx_ = nullptr;
    bool owned_ = false;
};

// Which frames a frame is compared with, over hm_find_frames_batch_device: VSlamData::find_visually_similar_and_recent_frames
// (cv-sfm/src/lib.rs:597-668) and the order try_localize gives its reconstructions (:853-855), for a batch of queries on the
// matcher's stream.  The frame table is the caller's device memory (the layouts are include/akz.h's); this class keeps its five
// addresses, its capacity and its row count.  This header knows no HIP: the rows' feed / pos / recon / view words are copied by
// the caller to the addresses append_rows / set_views hand out; the hashes are written by hm_hash_bag_device, whose d_hash is the
// tail.  find enqueues and returns.
class FrameIndex {
public:
    enum Verdict : uint32_t { Ok = HM_PL_OK, BadIndex = HM_PL_BAD_INDEX, BadTable = HM_PL_BAD_TABLE };
    struct Rows {              // the addresses of rows [first, first + count) in the five arrays
        uint32_t first, count;
        void *hashes, *feed, *pos, *recon, *view;
    };
    FrameIndex(space::Matcher& m, void* d_hashes, void* d_feed, void* d_pos, void* d_recon, void* d_view, uint32_t capacity, uint32_t hash_bytes)
        : m_(m), hashes_(d_hashes), feed_(d_feed), pos_(d_pos), recon_(d_recon), view_(d_view), capacity_(capacity), hb_(hash_bytes)
    {
        akaze::require_abi();
        if (hash_bytes == 0 || hash_bytes % 4 || hash_bytes > HM_PL_MAX_HASH_BYTES) throw std::invalid_argument("hash_bytes");
    }
    static hm_place_params params()
    {
        hm_place_params p;
        akaze::check(hm_place_params_default(&p), "hm_place_params_default");
        return p;
    }
    static uint32_t room(const hm_place_params& p) { return hm_place_room(&p); }
    uint32_t size() const { return n_; }
    // k frames appended in insertion order -> where their rows lie (hashes: the d_hash of hm_hash_bag_device); they have no view
    // until set_views: the caller writes HM_PL_NONE to their recon words with the feed and pos
    Rows append_rows(uint32_t k)
    {
        if (k > capacity_ - n_) throw std::length_error("FrameIndex: capacity");
        const Rows r = rows(n_, k);
        n_ += k;
        return r;
    }
    // Frame::view of stored rows [first, first + k): where the caller copies their reconstruction and view keys
    Rows set_views(uint32_t first, uint32_t k) const
    {
        if (first > n_ || k > n_ - first) throw std::out_of_range("FrameIndex: stored rows only");
        return rows(first, k);
    }
    void find(const void* d_query, const void* d_visible, uint32_t nq, const hm_place_params& p, uint32_t room, void* d_found, void* d_views_out,
              void* d_group_recon, void* d_group_start, void* d_free, void* d_search, void* d_counts, void* d_verdict,
              void* stream_to_wait = nullptr)
    {
        akaze::check(hm_find_frames_batch_device(m_.handle(), hashes_, feed_, pos_, recon_, view_, n_, hb_, d_query, d_visible, nq, &p, room, d_found,
                                                 d_views_out, d_group_recon, d_group_start, d_free, d_search, d_counts, d_verdict, stream_to_wait),
                     "hm_find_frames_batch_device");
    }
    // From a find's outputs to the searches, no host step in between (include/akz.h: hm_view_plan_device and the two planned
    // calls).  A frame takes the views of ONE found reconstruction — try_localize's turn (cv-sfm/src/lib.rs:858-891: d_pick null
    // = the first, else the ordinal) or, by_recon, the named one (.remove(&reconstruction), :926-939) — at most n_views of them.
    enum PlanVerdict : uint32_t {
        PlanOk = HM_VP_OK, PlanCut = HM_VP_CUT, NoGroup = HM_VP_NO_GROUP, FindRefused = HM_VP_FIND_REFUSED, BadView = HM_VP_BAD_VIEW,
        NoRoom = HM_VP_NO_ROOM
    };
    struct ViewPlan {          // device addresses, the caller's: [n_frames][n_views], [n_frames], [n_frames], [HM_VP_COUNTS] u32
        void *view_idx, *n_views_of, *verdict, *counts;
        uint32_t n_frames, n_views, n_blocks, exp_blocks;
    };
    void plan_views(const void* d_views_out, const void* d_group_recon, const void* d_group_start, const void* d_counts, const void* d_verdict,
                    uint32_t room, const void* d_pick, bool by_recon, const ViewPlan& plan, void* stream_to_wait = nullptr)
    {
        akaze::check(hm_view_plan_device(m_.handle(), d_views_out, d_group_recon, d_group_start, d_counts, d_verdict, room, d_pick,
                                         by_recon ? (uint32_t)HM_VP_PICK_RECON : 0u, plan.n_frames, plan.n_views, plan.n_blocks, plan.exp_blocks,
                                         plan.view_idx, plan.n_views_of, plan.verdict, plan.counts, stream_to_wait),
                     "hm_view_plan_device");
    }
    // the k nearest of every feature of the frames' blocks iq [n_frames] (host) in every view of their lists: d_out
    // [n_frames][n_views][cap][k]; slabs behind a frame's list are not written
    void knn_planned(const void* d_descs, const void* d_counts, uint32_t cap_per_img, const uint32_t* iq, const ViewPlan& plan, uint32_t k,
                     void* d_out, void* stream_to_wait = nullptr)
    {
        akaze::check(hm_knn_planned_batch_device(m_.handle(), d_descs, d_counts, d_descs, d_counts, cap_per_img, iq, plan.view_idx, plan.n_views_of,
                                                 plan.n_frames, plan.n_views, plan.n_blocks, plan.exp_blocks, k, d_out, stream_to_wait),
                     "hm_knn_planned_batch_device");
    }
    // register_frame_subset's landmark choice (:1489-1542) over those lists: d_best [n_frames][cap][3], d_decision [n_frames][cap]
    void best_of_views_planned(const void* d_knn, const void* d_counts, uint32_t cap_per_img, const uint32_t* iq, const ViewPlan& plan, uint32_t k,
                               const void* d_landmarks, uint32_t better_by, void* d_best, void* d_decision, void* stream_to_wait = nullptr)
    {
        akaze::check(hm_best_of_views_planned_batch_device(m_.handle(), d_knn, d_counts, iq, cap_per_img, plan.view_idx, plan.n_views_of,
                                                           plan.n_frames, plan.n_views, plan.n_blocks, k, d_landmarks, d_counts, better_by, d_best,
                                                           d_decision, stream_to_wait),
                     "hm_best_of_views_planned_batch_device");
    }
    void sync() { akaze::check(hm_sync(m_.handle()), "hm_sync"); }
    void* stream() { return hm_stream(m_.handle()); }

private:
    Rows rows(uint32_t first, uint32_t k) const
    {
        auto at = [first](void* base, std::size_t width) { return static_cast<void*>(static_cast<char*>(base) + width * first); };
        return Rows{first, k, at(hashes_, hb_), at(feed_, 4), at(pos_, 4), at(recon_, 4), at(view_, 4)};
    }
    space::Matcher& m_;
    void *hashes_, *feed_, *pos_, *recon_, *view_;
    uint32_t capacity_, hb_, n_ = 0;
};
}  // namespace cv_sfm

// hamming_lsh::HammingHasher<64, H> and the lsh_to_frame map of cv-sfm (cv-sfm/src/lib.rs:205-217, 672, 622-624) over
// hm_hash_bag / hm_hash_knn.  The hashing crate is not vendored in the reference: see oracle/lsh_oracle.c for what
// is restated (nearest-codeword bag hash, one bit per codeword).
namespace hamming_lsh {

class HammingHasher {
public:
    // new_with_codewords: codewords.size() = 8 x hash bytes (4096 for cv-sfm's BitArray<512>)
    HammingHasher(std::vector<akaze::BitArray64> codewords, space::Matcher& m) : cw_(std::move(codewords)), m_(m)
    {
        if (cw_.empty() || cw_.size() % 32) throw std::invalid_argument("codeword count must be a multiple of 32");
    }
    std::size_t hash_bytes() const { return cw_.size() / 8; }
    // hash_bag(features) -> BitArray<H> as bytes
    std::vector<uint8_t> hash_bag(const std::vector<akaze::BitArray64>& features) const
    {
        std::vector<uint8_t> h(hash_bytes());
        akaze::check(hm_hash_bag(m_.handle(), reinterpret_cast<const akz_descriptor*>(features.data()),
                                 (uint32_t)features.size(), reinterpret_cast<const akz_descriptor*>(cw_.data()),
                                 (uint32_t)cw_.size(), h.data(), nullptr),
                     "hm_hash_bag");
        return h;
    }

private:
    std::vector<akaze::BitArray64> cw_;
    space::Matcher& m_;
};

// insert(hash, value) / knn_values(hash, num): exact nearest hashes in (distance, insertion order)
template <typename V>
class HashIndex {
public:
    HashIndex(std::size_t hash_bytes, space::Matcher& m) : hb_(hash_bytes), m_(m) {}
    void insert(const std::vector<uint8_t>& hash, V value)
    {
        if (hash.size() != hb_) throw std::invalid_argument("hash size");
        store_.insert(store_.end(), hash.begin(), hash.end());
        values_.push_back(std::move(value));
    }
    std::vector<std::pair<space::Neighbor, V>> knn_values(const std::vector<uint8_t>& hash, std::size_t num) const
    {
        std::vector<akz_neighbor> out(num ? num : 1);
        uint32_t n = 0;
        akaze::check(hm_hash_knn(m_.handle(), hash.data(), store_.data(), (uint32_t)values_.size(), (uint32_t)hb_,
                                 (uint32_t)num, out.data(), &n),
                     "hm_hash_knn");
        std::vector<std::pair<space::Neighbor, V>> r;
        for (uint32_t i = 0; i < n; ++i) r.push_back({space::Neighbor{out[i].index, out[i].distance}, values_[out[i].index]});
        return r;
    }

private:
    std::size_t hb_;
    space::Matcher& m_;
    std::vector<uint8_t> store_;
    std::vector<V> values_;
};

}  // namespace hamming_lsh
