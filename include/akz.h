/* akz.h — C ABI of the MI355X-native AKAZE + brute-force Hamming front-end.
 *
 * This is the drop-in boundary for the reference's data-parallel hot path.
 * Every entry point names the reference interface it replaces (paths relative to the rust-cv/cv
 * checkout).  Plain pointers and sizes only: no C++/torch/HIP types appear in a signature
 * (device pointers and streams travel as void*).
 *
 * Conventions
 *   - every function returns an int32_t status: AKZ_OK (0) or a negative akz_status;
 *     nothing throws, nothing aborts, akz_strerror() names the code;
 *   - the library never retains a caller pointer after the call returns;
 *   - a context is bound to one HIP device and one internal stream; use one context per host
 *     thread.  Contexts on different devices are independent;
 *   - "capacity" arguments are in elements.  When an output does not fit, the call returns
 *     AKZ_E_CAPACITY and *n_out holds the required element count;
 *   - there is NO CPU fallback: if no HIP device is usable akz_create() fails with AKZ_E_NO_DEVICE.
 */
#ifndef AKZ_H
#define AKZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum akz_status {
    AKZ_OK = 0,
    AKZ_E_INVALID = -1,    /* null pointer, bad dimension, unsupported config value */
    AKZ_E_NO_DEVICE = -2,  /* no usable HIP device / device index out of range */
    AKZ_E_OOM = -3,        /* hipMalloc failed */
    AKZ_E_CAPACITY = -4,   /* caller buffer too small; *n_out = required */
    AKZ_E_HIP = -5,        /* a HIP runtime call failed (akz_last_hip_error()) */
    AKZ_E_TOO_LARGE = -6,  /* image or batch exceeds what the context was created for */
    AKZ_E_INTERNAL = -7,   /* device-side overflow of an internal work list */
    AKZ_E_COMM = -8        /* an RCCL call failed, or librccl.so.1 could not be loaded (akz_comm_*) */
} akz_status;

/* akaze::Akaze — akaze/src/lib.rs:109-142 (fields), :169-185 (Default), :147-166 (new/sparse/dense).
 * Field-for-field; usize -> uint64_t. */
typedef struct akz_config {
    uint64_t maximum_features;        /* usize::MAX by default */
    uint32_t num_sublevels;           /* 4 */
    uint32_t max_octave_evolution;    /* 4 */
    double base_scale_offset;         /* 1.6 */
    double initial_contrast;          /* 0.001 (unused by the reference as well) */
    double contrast_percentile;       /* 0.7 */
    uint64_t contrast_factor_num_bins; /* 300 */
    double derivative_factor;         /* 1.5 */
    double detector_threshold;        /* 0.001; sparse 0.01; dense 0.0001 */
    uint64_t descriptor_channels;     /* 3 */
    uint64_t descriptor_pattern_size; /* 10 */
} akz_config;

/* `stream_to_wait` arguments (a hipStream_t passed as void*): the stream that produced the call's device inputs; the
 * library's stream waits for the work enqueued on it so far.  NULL = nothing to wait for.  The legacy default stream's
 * own handle is NULL as well, so a caller that enqueues on it (torch without a stream context, plain `<<<>>>` launches)
 * passes AKZ_STREAM_LEGACY — the value of hipStreamLegacy — instead: the library's streams are non-blocking and do NOT
 * synchronise with the default stream on their own.
 *
 * What "returns after enqueueing" means for the `*_device` entries.  A call orders its work behind stream_to_wait and returns
 * while that stream may still be busy; a host index list (`const uint32_t*`) has been read when the call returns, and the
 * caller may overwrite or free it.  A call waits on the host in these cases only, and its results are the same when it does:
 *   - rs_* and hm_* entries keep scratch in their context that grows to the largest call so far: a call that needs more than
 *     the context holds waits for the context's stream — and so for stream_to_wait — before it frees and reallocates.  A
 *     context in steady use has seen its sizes, and does not wait.
 *   - hm_* entries that take host lists or build problem descriptors stage them through a ring of four pinned slots, each
 *     sized on its first use (one such wait per slot, and again when a slot has to grow).  A fifth call while the copies of the
 *     four before it are still held up waits for the oldest of them: the ring lets the host run four calls ahead, not more.
 *   - the rs_* entries copy their host lists from the caller's pageable memory with hipMemcpyAsync.  On the ROCm runtime this
 *     was measured on, the copy of a list of a few words is staged at once and the call returns; the library does not control
 *     that ("Enqueue contract"). */
#define AKZ_STREAM_LEGACY ((void*)1)

/* akaze::KeyPoint — akaze/src/lib.rs:69-93. point=(x,y). 28 bytes, no padding. */
typedef struct akz_keypoint {
    float x, y;
    float response;
    float size;
    float angle;
    uint32_t octave;
    uint32_t class_id;
} akz_keypoint;

/* bitarray::BitArray<64> as filled by akaze/src/descriptors.rs:181-202: bit i lives in
 * bytes[i >> 3] at position (i & 7); 486 bits used, bits 486..511 are zero. */
typedef struct akz_descriptor {
    uint8_t bytes[64];
} akz_descriptor;

/* space::Neighbor<u32> — what LinearKnn::knn returns (call sites akaze/tests/estimate_pose.rs:82-88,
 * tutorial-code/chapter5-geometric-verification/src/main.rs:155-161). */
typedef struct akz_neighbor {
    uint32_t index;
    uint32_t distance;
} akz_neighbor;

typedef struct akz_ctx akz_ctx;

/* Akaze::default() (akaze/src/lib.rs:169-185). */
void akz_config_default(akz_config* cfg);

/* Context = the pre-allocated per-device pyramid for up to max_batch frames of up to
 * max_w x max_h pixels (what Akaze::allocate_evolutions, akaze/src/evolution.rs:80-126, allocates
 * per call in the reference).  max_keypoints bounds the per-frame candidate/keypoint lists
 * (0 = default 16384).  max_w, max_h in [3, 65535] and max_w * max_h <= 2^28 pixels (the kernels address a
 * frame's planes with 32-bit byte offsets): a larger frame is refused with AKZ_E_TOO_LARGE. */
int32_t akz_create(const akz_config* cfg, int32_t device, int32_t max_w, int32_t max_h,
                   int32_t max_batch, uint32_t max_keypoints, akz_ctx** out);
int32_t akz_destroy(akz_ctx* ctx);

/* Behaviour switches of ONE context.  The library reads no environment variable: two contexts in one
 * process can differ, and nothing outside the caller's code changes what a context does.  The defaults
 * (all zero) are the measured-best paths; the other values select the fall-back / reference kernels that
 * the parity tests and A/B runs exercise.  Results are bit-identical under every combination (of everything but `arith`, below). */
enum {
    AKZ_OPT_KEEP_ALL = 1u << 0,           /* keep per-level Lsmooth / Lflow and write the Ldet planes (parity taps) */
    AKZ_OPT_NO_FRAME_PAIRS = 1u << 1,     /* one-frame kernels even for widths divisible by 4 */
    AKZ_OPT_SERIAL_SUPPRESSION = 1u << 2, /* one-wave serial walk of scale_space_extrema.rs:61-118 for every frame */
    AKZ_OPT_NO_PIPELINE = 1u << 3,        /* one buffer set: consecutive calls do not overlap */
    AKZ_OPT_STREAM_PRIORITY = 1u << 4,    /* (accepted, no effect: scale-space stream at high and keypoint stream at low
                                           * priority is the default since it measured +1 % on the bench workload) */
    AKZ_OPT_CONTRAST_EXACT = 1u << 5,     /* contrast factor always through the exact histogram pass */
    AKZ_OPT_CONTRAST_FORCE_ODD = 1u << 6, /* test knob: odd frames through the exact pass (mixed pairs) */
    AKZ_OPT_TILE_KERNELS = 1u << 7,       /* the LDS-tile determinant kernels of round 1 instead of the row-streaming one */
    AKZ_OPT_SERIAL_DET = 1u << 8,         /* determinant / candidate kernels on the scale-space stream itself instead of
                                           * the side stream that takes them off the Lt -> Lt dependency chain */
    AKZ_OPT_SPLIT_FRONT_FED = 1u << 9,    /* level front end and first FED launch as two kernels (Lflow through HBM)
                                           * instead of the fused k_front_fed */
    AKZ_OPT_EQUAL_PRIORITY = 1u << 10,    /* all streams of the context at the default priority */
    AKZ_OPT_NO_RESIDENT_LEVELS = 1u << 11 /* the tile kernels (k_front_fed + k_fed_pair launches) also for the levels small enough
                                           * to live on one compute unit, instead of k_level_resident */
};
typedef struct akz_options {
    uint32_t struct_size;     /* sizeof(akz_options) of the caller (lets the struct grow) */
    uint32_t flags;           /* AKZ_OPT_* */
    uint32_t fed_block;       /* most FED steps fused per launch, 1..8; 0 = default (8; the first octave stops at 4) */
    uint32_t sup_capacity;    /* candidates per frame the parallel suppression is sized for; 0 = 4 x max_keypoints */
    uint32_t max_candidates;  /* capacity of each per-(frame, level) extrema candidate list; 0 = max_keypoints */
    uint32_t desc_tile_shift; /* log2 tile edge of the descriptor visiting order, 2..9; 0 = default (5) */
    uint32_t stream_waves;    /* waves a row-streaming launch aims for (sets its row-segment length); 0 = default (8192) */
    uint32_t stream_min_waves; /* launches that cannot field this many streaming waves take the tile kernel; 0 = default (2048) */
    uint32_t arith;           /* AKZ_ARITH_* bits: which of the reference's un-vendored arithmetic orders the filters use; 0 = default */
    uint32_t cu_ss;           /* CU partitioning (hipExtStreamCreateWithCUMask), 0 = none: the scale-space and determinant streams run on the */
    uint32_t cu_kp;           /* FIRST cu_ss compute units of every XCD, the keypoint stream on the LAST cu_kp (1..32 each; measured: DESIGN.md 5).
                               * Experiment-only: a masked stream is created by an API that takes neither a priority nor
                               * hipStreamNonBlocking, so it OVERRIDES AKZ_OPT_EQUAL_PRIORITY (no priorities at all) and is a
                               * blocking stream — it synchronises implicitly with the NULL stream of the process.  The same
                               * holds for HM_OPT_CU_MASK against HM_OPT_STREAM_PRIORITY. */
    uint32_t resident_min_frames; /* fewest frames of a call for which k_level_resident (one workgroup per frame) takes the levels that
                               * fit one compute unit; 0 = default (3/8 of the device's compute units: a call of fewer frames leaves
                               * most of the chip idle under it and keeps the tile kernels); 1 = always (tests) */
    uint32_t reserved[4];     /* must be zero */
} akz_options;
/* akz_options.arith — the only option that CHANGES RESULTS.  Three pieces of the reference's arithmetic live in crates that
 * are not vendored in rust-cv/cv, and its known answers (399 / 343 descriptors, 11 matches) come out the same under all
 * eight combinations, so none can be ruled out from here:
 *   wide::f32x4::reduce_add of the four filter lanes (akaze/src/image.rs:246-247, :324-325):  ((a0 + a1) + a2) + a3  [default]
 *                                                                                     or  (a0 + a1) + (a2 + a3)   [REDUCE_PAIRWISE]
 *   wide::f32x4::mul_add in the filters' accumulation (image.rs:246, :324):  multiply, then add  [default]  or one fused operation [FMA]
 *   ndarray's sum() over a 2 x 2 window in half_size (image.rs:160-166):     (a + b) + (c + d)   [default]  or  ((a + b) + c) + d  [HALF_SEQUENTIAL]
 * The default is what the crate sources imply for a default x86-64 build.  Every combination is a complete copy of the
 * scale-space kernels (no cost in the default one) and is held bit for bit to the oracle under the same ORC_OPT_* switches. */
enum { AKZ_ARITH_REDUCE_PAIRWISE = 1u << 0, AKZ_ARITH_FMA = 1u << 1, AKZ_ARITH_HALF_SEQUENTIAL = 1u << 2 };
/* akz_create with explicit options (NULL = defaults = akz_create). */
int32_t akz_create_ex(const akz_config* cfg, int32_t device, int32_t max_w, int32_t max_h,
                      int32_t max_batch, uint32_t max_keypoints, const akz_options* opts, akz_ctx** out);

/* Akaze::extract on a DynamicImage::ImageLuma8 (akaze/src/lib.rs:295, image.rs:47-56):
 * img is host memory, h rows of w bytes, `stride` bytes apart.  Outputs are index-aligned,
 * ordered by response descending, exactly as the reference returns them. */
int32_t akz_extract_gray_u8(akz_ctx* ctx, const uint8_t* img, int32_t w, int32_t h, int32_t stride,
                            akz_keypoint* kps, akz_descriptor* descs, uint32_t cap, uint32_t* n_out);

/* Akaze::extract on a DynamicImage::ImageLuma16 (akaze/src/image.rs:57-66: f32::from(v) / 65535f32 per
 * pixel); stride in elements. */
int32_t akz_extract_gray_u16(akz_ctx* ctx, const uint16_t* img, int32_t w, int32_t h, int32_t stride,
                             akz_keypoint* kps, akz_descriptor* descs, uint32_t cap, uint32_t* n_out);

/* Akaze::extract_from_gray_float_image (akaze/src/lib.rs:309): f32 pixels in [0,1], stride in
 * elements. */
int32_t akz_extract_gray_f32(akz_ctx* ctx, const float* img, int32_t w, int32_t h, int32_t stride,
                             akz_keypoint* kps, akz_descriptor* descs, uint32_t cap, uint32_t* n_out);

/* Akaze::extract on a COLOUR DynamicImage (akaze/src/image.rs:45-46: `input_image.grayscale()` first): 8- and 16-bit
 * RGB(A) become Luma8 / Luma16 by the `image` crate's integer Rec. 709 luma, (2126 R + 7152 G + 722 B) / 10000
 * truncating, and take the arms of image.rs:47-66; Rgb32F / Rgba32F keep their floats and take `to_luma()` per pixel
 * (image.rs:87-106: the same weights in f64, narrowed to f32).  The `image` crate is not vendored in the reference:
 * colour-input parity is unpinned (oracle/color_oracle.c restates the published formula).  pixels: host memory, h rows
 * of `stride` ELEMENTS, `channels` = 3 or 4 interleaved samples per pixel (alpha ignored); fmt = AKZ_FMT_* of a sample. */
int32_t akz_extract_color(akz_ctx* ctx, const void* pixels, int32_t fmt, int32_t channels, int32_t w, int32_t h, int32_t stride,
                          akz_keypoint* kps, akz_descriptor* descs, uint32_t cap, uint32_t* n_out);

/* Pixel formats of the batched / device entry points: the arms of GrayFloatImage::from_dynamic
 * (akaze/src/image.rs:45-109) that need no colour conversion. */
enum { AKZ_FMT_U8 = 0 /* Luma8: v / 255 */, AKZ_FMT_F32 = 1 /* GrayFloatImage, [0,1] */, AKZ_FMT_U16 = 2 /* Luma16: v / 65535 */ };

/* Batched extract: n host images of identical size (what a caller looping Akaze::extract over
 * frames does, cv-sfm/src/lib.rs:2200-2204).  fmt: AKZ_FMT_*; stride in elements.  kps/descs hold
 * n * cap_per_img entries, frame i at offset i*cap_per_img; n_out[i] = count of frame i. */
int32_t akz_extract_batch(akz_ctx* ctx, const void* const* imgs, int32_t fmt, int32_t n, int32_t w,
                          int32_t h, int32_t stride, akz_keypoint* kps, akz_descriptor* descs,
                          uint32_t cap_per_img, uint32_t* n_out);

/* Zero-copy batched extract for a device-resident pipeline: d_imgs is ONE device buffer of n
 * frames (frame-major, tightly packed w*h elements each), outputs are device buffers laid out
 * as in akz_extract_batch; d_n_out is a device array of n counts.  Work is enqueued on the
 * context's stream; `stream_to_wait` (a hipStream_t passed as void*, may be NULL) is the stream
 * that produced d_imgs.  The call returns after enqueueing; akz_sync() waits. */
int32_t akz_extract_batch_device(akz_ctx* ctx, const void* d_imgs, int32_t fmt, int32_t n, int32_t w,
                                 int32_t h, void* d_kps, void* d_descs, uint32_t cap_per_img,
                                 void* d_n_out, void* stream_to_wait);
int32_t akz_sync(akz_ctx* ctx);
/* The context's hipStream_t, as void*, so callers can order their own work after ours. */
void* akz_stream(akz_ctx* ctx);

/* Scale-space only (BASELINE.json configs[1] "scale-space kernels only"): runs A1..A11 of
 * SURVEY.md §8a — create_nonlinear_scale_space (akaze/src/lib.rs:193-258) + detector_response
 * (akaze/src/detector_response.rs:33-57) — on n device-resident frames and leaves Lt/Lx/Ly/Ldet
 * of every level in the context. */
int32_t akz_scale_space_device(akz_ctx* ctx, const void* d_imgs, int32_t fmt, int32_t n, int32_t w,
                               int32_t h, void* stream_to_wait);

/* After a call answered AKZ_E_INTERNAL: which internal list of which frame of that batch overflowed, and what it
 * would have needed (the reference's Vecs grow without bound, akaze/src/lib.rs:169-171 maximum_features =
 * usize::MAX; here every list has a capacity fixed at akz_create_ex: max_keypoints per frame — at most 262144 — and
 * akz_options.max_candidates raw extrema per (frame, level)).  flags bit 0: a per-level candidate list (needed_candidates
 * = the longest list of the frame); bit 1: the frame's keypoint lists after suppression. */
typedef struct akz_overflow_info {
    uint32_t flags;
    uint32_t needed_candidates;   /* largest per-level extrema count of the frame */
    uint32_t candidate_capacity;
    uint32_t keypoint_capacity;
} akz_overflow_info;
int32_t akz_last_overflow(akz_ctx* ctx, akz_overflow_info* per_frame, uint32_t cap, uint32_t* n_frames);

/* ---- pyramid introspection / parity taps (what Akaze::allocate_evolutions returns) ---- */
typedef struct akz_level_info {
    int32_t width, height;
    uint32_t octave, sublevel;
    double esigma, etime;
    uint32_t n_fed_steps;
    uint32_t deriv_sigma; /* round(esigma*derivative_factor/2^octave), detector_response.rs:11-13 */
} akz_level_info;
int32_t akz_num_levels(akz_ctx* ctx, int32_t w, int32_t h, int32_t* n_levels);
int32_t akz_level(akz_ctx* ctx, int32_t w, int32_t h, int32_t level, akz_level_info* out);
int32_t akz_fed_tau(akz_ctx* ctx, int32_t w, int32_t h, int32_t level, double* tau, uint32_t cap,
                    uint32_t* n_out);
enum { AKZ_BUF_LT = 0, AKZ_BUF_LSMOOTH = 1, AKZ_BUF_LX = 2, AKZ_BUF_LY = 3, AKZ_BUF_LDET = 4,
       AKZ_BUF_LFLOW = 5 };
/* Copy one level buffer of frame `img` of the most recent batch to host `out` (w*h floats). */
int32_t akz_debug_get_level(akz_ctx* ctx, int32_t img, int32_t level, int32_t which, float* out);
/* Contrast factor (compute_contrast_factor, akaze/src/contrast_factor.rs:16-64) of frame img. */
int32_t akz_debug_get_contrast(akz_ctx* ctx, int32_t img, double* out);
/* Keypoint list after a named stage of frame img of the most recent batch:
 * 0 = find_scale_space_extrema output (scale_space_extrema.rs:14-143),
 * 1 = after do_subpixel_refinement + orientation (:297-362), 2 = after sort+truncate (lib.rs:326-327). */
int32_t akz_debug_get_keypoints(akz_ctx* ctx, int32_t img, int32_t stage, akz_keypoint* out,
                                uint32_t cap, uint32_t* n_out);

/* The transcendentals of the orientation and descriptor stages as the DEVICE evaluates them (f32::atan2 at
 * scale_space_extrema.rs:242, f32::cos / sin at descriptors.rs:70-71): which 0: out = atan2f(y, x); 1: sinf(x); 2: cosf(x)
 * (y ignored).  Host buffers.  The tests hold these to the host libm within 1 ulp. */
int32_t akz_debug_portable_math(akz_ctx* ctx, int32_t which, const float* x, const float* y, uint32_t n, float* out);

/* Window membership of orientation samples (weighted gradient (x[i], y[i]); scale_space_extrema.rs:242-287), bit w = the
 * sample's angle lies in window w: fast[i] as the descriptor kernel decides it (an f32 estimate of the angle, the exact
 * expression inside a band around the windows' end points), exact[i] from the exact expression alone, fell_back[i] = 1 where
 * the band applied.  fast == exact for every input is the kernel's contract; the tests drive this with end points +- a few
 * ulp, axes, zeros, denormals and huge operands.  Host buffers. */
int32_t akz_debug_orientation_masks(akz_ctx* ctx, const float* x, const float* y, uint32_t n, uint64_t* fast, uint64_t* exact,
                                    uint32_t* fell_back);
/* The error BOUND of that estimate (tools/ubench/atan_bound.c, tests/test_oracle_math.py: 1.84e-6 in total against the band
 * of 8e-6) takes one thing from the instruction set's specification: v_rcp_f32 is accurate to 1 ulp.  This checks it on the
 * device in use: the instruction against 1 / x in f64 for EVERY f32 whose bit pattern lies in [lo_bits, hi_bits] (positive
 * normal numbers); *max_ulps = the largest error in ulps of the correctly rounded quotient. */
int32_t akz_debug_rcp_error(akz_ctx* ctx, uint32_t lo_bits, uint32_t hi_bits, double* max_ulps);

/* ---- stand-alone image ops (akaze::image public API, akaze/src/image.rs:202-389) ---- */
/* gaussian_kernel(r, kernel_size) — image.rs:360-374.  Host-only scalar math. */
int32_t akz_gaussian_kernel(float r, uint32_t kernel_size, float* out);
/* horizontal_filter / vertical_filter / separable_filter — image.rs:202-340: clamp-border
 * correlation with the reference's 4-lane accumulation order.  Host buffers in and out. */
int32_t akz_horizontal_filter(akz_ctx* ctx, const float* img, int32_t w, int32_t h,
                              const float* kernel, uint32_t ksize, float* out);
int32_t akz_vertical_filter(akz_ctx* ctx, const float* img, int32_t w, int32_t h,
                            const float* kernel, uint32_t ksize, float* out);
/* GrayFloatImage::half_size — image.rs:154-199. out is (w/2)*(h/2). */
int32_t akz_half_size(akz_ctx* ctx, const float* img, int32_t w, int32_t h, float* out);

/* ---- brute-force Hamming matcher (space::LinearKnn{metric: Hamming} + bitarray::BitArray<64>) ---- */
/* Bicubic colour sampling at keypoints: cv-sfm/src/bicubic.rs:34-68 (interpolate_bicubic) as called by
 * VSlam::kps_descriptors (cv-sfm/src/lib.rs:2207-2216) on image.to_rgb8() at kp.point.  rgb: host, h rows of
 * `stride` bytes, 3 bytes per pixel; colors [n][3].  A 4x4 neighbourhood that leaves the image gives the
 * reference's default [0,0,0]. */
int32_t akz_sample_colors_rgb8(akz_ctx* ctx, const uint8_t* rgb, int32_t w, int32_t h, int32_t stride,
                               const akz_keypoint* kps, uint32_t n, uint8_t* colors);
/* The same lookup for a whole micro-batch, where the data already lies on the device: d_rgb [n] RGB8 images of h rows of
 * `stride` bytes (an image is h * stride bytes), d_kps [n][cap_per_img] akz_keypoint and d_counts [n] u32 as
 * akz_extract_batch_device leaves them.  d_colors [n][cap_per_img][3] u8: feature j < min(count, cap_per_img) of frame f gets
 * interpolate_bicubic at its point; the rows at or behind the count are not written.  n within [1, 65535], stride >= 3 * w, else
 * AKZ_E_INVALID (decided before the context is looked at).  One launch on akz_stream() — the stream the extraction's outputs
 * complete on — after stream_to_wait (may be NULL); returns after enqueueing; allocates nothing. */
int32_t akz_sample_colors_batch_device(akz_ctx* ctx, const void* d_rgb, int32_t n, int32_t w, int32_t h, int32_t stride, const void* d_kps,
                                       const void* d_counts, uint32_t cap_per_img, void* d_colors, void* stream_to_wait);

typedef struct hm_ctx hm_ctx;
int32_t hm_create(int32_t device, uint32_t max_queries, uint32_t max_targets, hm_ctx** out);
/* hm_create with kernel-selection flags (0 = defaults): the k-NN kernel is the FP4 MFMA one (64 resident queries per
 * wave, target tiles by LDS-DMA) unless a flag selects its register-staged predecessor (HM_OPT_NO_LDS_DMA), the int8
 * MFMA or the xor/popcount VALU kernel (k = 2 only); all four are bit-identical. */
enum { HM_OPT_NO_FP4 = 1u << 0, HM_OPT_NO_MFMA = 1u << 1, HM_OPT_STREAM_PRIORITY = 1u << 2, HM_OPT_NO_LDS_DMA = 1u << 3,
       HM_OPT_CU_SHIFT = 16, HM_OPT_CU_MASK = 0x3Fu << 16 /* bits 16..21: the matcher's stream on the LAST n compute units of every XCD (0 = all) */,
       /* The reverse side of a symmetric match (hm_match, hm_match_batch_device; rules BETTER_BY_STRICT, and BETTER_BY with
        * param_u >= 1).  Default: per problem, answered from the forward lists where that asks for at most a share of na * nb
        * explicit distances, by the reverse 2-NN search otherwise — decided on the device, same pairs either way.
        * HM_OPT_REVERSE_SEARCH: always the search; HM_OPT_REVERSE_LISTS: never (the two exclude each other: AKZ_E_INVALID).
        * Bits 8..12: n > 0 sets the share to 2^-n (0: the built-in 1/4). */
       HM_OPT_REVERSE_SEARCH = 1u << 4, HM_OPT_REVERSE_LISTS = 1u << 5, HM_OPT_REVERSE_SHARE_SHIFT = 8, HM_OPT_REVERSE_SHARE_MASK = 0x1Fu << 8 };
int32_t hm_create_ex(int32_t device, uint32_t max_queries, uint32_t max_targets, uint32_t flags, hm_ctx** out);
int32_t hm_destroy(hm_ctx* ctx);
/* LinearKnn::knn(q, 2) for every query (akaze/tests/estimate_pose.rs:82-88): out[2*i+0/1] are the
 * nearest and second-nearest targets of query i under Hamming distance over all 64 bytes, ordered
 * by (distance, index) ascending — the lowest index wins ties.  nt < 2 is AKZ_E_INVALID (the
 * reference asserts two neighbours, estimate_pose.rs:89). Host buffers. */
int32_t hm_knn2(hm_ctx* ctx, const akz_descriptor* q, uint32_t nq, const akz_descriptor* t,
                uint32_t nt, akz_neighbor* out);
/* LinearKnn{metric: Hamming, iter: t}.knn(q, k) for k = 1, 2 or 3 — the registration path asks for 3
 * (cv-sfm/src/lib.rs:1474).  out[nq][k], ascending (distance, index); the reference returns min(k, nt)
 * neighbours, here the slots past nt hold {index 2^22 - 1, distance 1023}.  The distance is over all 512 bits of both rows:
 * an extracted descriptor has bits 486..511 clear, but a row that sets them (a codeword, a hash, any caller's BitArray<64>) has
 * them counted like every other bit, in every kernel, so distances reach 512. */
int32_t hm_knn(hm_ctx* ctx, const akz_descriptor* q, uint32_t nq, const akz_descriptor* t, uint32_t nt,
               uint32_t k, akz_neighbor* out);
/* LinearKnn keeps its targets (`iter`) and is asked once per query (akaze/tests/estimate_pose.rs:82-88).  hm_set_targets
 * uploads the target set once; hm_knn_targets answers queries — one, or a batch — against the resident copy, results as
 * hm_knn's.  Any other host-buffer call on the context (hm_knn, hm_knn2, hm_match, hm_hash_bag) reuses the staging buffer
 * and ends the residency: hm_knn_targets then returns AKZ_E_INVALID rather than search stale data. */
int32_t hm_set_targets(hm_ctx* ctx, const akz_descriptor* t, uint32_t nt);
/* The number of the hm_set_targets call whose targets the context holds, 0 when nothing is resident.  A LinearKnn mirror keeps
 * the value its own upload produced and compares before every hm_knn_targets: any other upload or residency-ending call on the
 * context in between changes it (a pointer / length comparison of the host array would not notice a re-used allocation). */
uint64_t hm_targets_generation(hm_ctx* ctx);
int32_t hm_knn_targets(hm_ctx* ctx, const akz_descriptor* q, uint32_t nq, uint32_t k, akz_neighbor* out);
/* Device-resident multi-view form of the same call (cv-sfm/src/lib.rs:1468-1486: every feature of the new
 * frame against each of up to 32 recent views): d_q [cap][64] + count d_nq, d_views [..][cap][64] + counts
 * d_nviews, view v of this call = block view_idx[v]; d_out [n_views][cap][k].  Stream-ordered after
 * stream_to_wait; results are complete on hm_stream().  The landmark bookkeeping that follows in the
 * reference (HashMap dedup, merge rules) is control plane and stays with the caller. */
int32_t hm_knn_views_device(hm_ctx* ctx, const void* d_q, const void* d_nq, const void* d_views,
                            const void* d_nviews, uint32_t cap_per_img, const uint32_t* view_idx,
                            uint32_t n_views, uint32_t k, void* d_out, void* stream_to_wait);
/* The batched form: problem p = every feature of query block iq[p] (of d_q, count d_nq[iq[p]]) against target block it[p]
 * (of d_t), k neighbours each — the window of recent views of every frame of a micro-batch (n_frames x K problems) in one
 * call; every distinct block is recoded once per count it is read with (d_q and d_t may be one buffer, with different counts
 * per side).  iq / it host index arrays, n_probs <= 65535; d_out [n_probs][cap][k], slots past
 * a target block's count as in hm_knn. */
int32_t hm_knn_batch_device(hm_ctx* ctx, const void* d_q, const void* d_nq, const void* d_t, const void* d_nt,
                            uint32_t cap_per_img, const uint32_t* iq, const uint32_t* it, uint32_t n_probs, uint32_t k,
                            void* d_out, void* stream_to_wait);
/* What follows hm_knn_views_device in the reference (cv-sfm/src/lib.rs:1489-1542): per feature, the best distance of
 * every distinct landmark among its n_views x k neighbours, the three best landmarks (ascending (distance, landmark
 * key): the reference's HashMap leaves the order of equal distances unspecified), and the decision of :1516-1532 —
 * 1: best[0] is a unique match (best[0].d + better_by <= best[1].d); 2: best[0], best[1] are merge candidates
 * (best[1].d + better_by <= best[2].d; the caller still applies are_landmarks_sharing_view); 0: neither, or fewer
 * than three distinct landmarks.  d_knn = hm_knn_views_device's d_out [n_views][cap][k]; d_landmarks
 * [view blocks][cap] u32 = the landmark key observed by each feature of each stored view (reconstruction.views[v]
 * .landmarks); d_best [cap][3] {landmark, distance} (0xFFFFFFFF when absent), d_decision [cap] u32. */
int32_t hm_best_of_views_device(hm_ctx* ctx, const void* d_knn, const void* d_nq, uint32_t cap_per_img,
                                const uint32_t* view_idx, uint32_t n_views, uint32_t k, const void* d_landmarks,
                                const void* d_nviews, uint32_t better_by, void* d_best, void* d_decision,
                                void* stream_to_wait);
/* The same for every frame of a micro-batch in one launch: d_knn = hm_knn_batch_device's output laid out
 * [n_frames][n_views][cap][k] (problem f * n_views + v = frame f against its v-th view), frame f's count d_nq[iq[f]], its views
 * view_idx[f * n_views + v]; d_best [n_frames][cap][3], d_decision [n_frames][cap].  n_frames <= 65535. */
int32_t hm_best_of_views_batch_device(hm_ctx* ctx, const void* d_knn, const void* d_nq, const uint32_t* iq, uint32_t cap_per_img,
                                      const uint32_t* view_idx, uint32_t n_frames, uint32_t n_views, uint32_t k,
                                      const void* d_landmarks, const void* d_nviews, uint32_t better_by, void* d_best,
                                      void* d_decision, void* stream_to_wait);
/* What follows the decision in register_frame_subset (cv-sfm/src/lib.rs:1516-1532, 1549-1563, 1583-1604), for every frame of
 * a micro-batch.  original_matches: a feature with decision 1 is the match ([best0], feature); a feature with decision 2
 * whose two landmarks share no view — are_landmarks_sharing_view (:1528) is the caller's graph test, its verdict is
 * d_merge_ok [n_frames][cap] u8 (non-zero: the merge may be attempted), NULL when no merge candidate passes — is the match
 * ([best0, best1], feature).  landmark_counts covers every landmark of every original match, both landmarks of a merge
 * included, and a match survives only if each of its landmarks was counted once (:1549-1563).  A survivor whose
 * triangulation is None is dropped (:1583-1604, filter_map): d_world is the table of homogeneous world points
 * (rs_triangulate_landmarks_device / rs_triangulate_merged_device make it on the device; a caller may bring its own),
 * rows [0, n_world) indexed by landmark key (triangulate_landmark_robust) and — only with a merge mask — rows
 * n_world + f * cap + j = triangulate_merged_landmark_robust of frame f's feature j; a row with w < 0 (impossible for a
 * Projective point) or a landmark key >= n_world says "None".  d_best / d_decision / d_nq / iq as
 * hm_best_of_views_batch_device wrote / took them; d_pairs [n_frames][cap][2] u32 {feature, world row} in ascending feature
 * order, d_npairs [n_frames] — the pair lists rs_p3p_arrsac_batch_device takes (with n_world + n_frames * cap rows when a
 * merge mask is given).  cap_per_img <= 8192.  (Ascending feature order: the order for a caller that shuffles the
 * matches itself, RS_BATCH_SHUFFLE; the reference's own order is the next entry point's.) */
int32_t hm_landmark_matches_batch_device(hm_ctx* ctx, const void* d_best, const void* d_decision, const void* d_merge_ok,
                                         const void* d_nq, const uint32_t* iq, uint32_t cap_per_img, uint32_t n_frames,
                                         const void* d_world, uint32_t n_world, void* d_pairs, void* d_npairs, void* stream_to_wait);
/* The same lists IN THE ORDER THE REFERENCE HANDS TO THE CONSENSUS (cv-sfm/src/lib.rs:1561-1574): original_matches is stably
 * sorted by Reverse(sum over the match's landmarks of landmark(..).observations.len()) before model_inliers (:1619-1622) sees
 * it — matches on well-observed landmarks first, equal sums in feature order — and a consensus that samples by position
 * (ARRSAC does) depends on it.  d_obs_counts [n_world] u32: observations of every landmark key (the caller's graph knows them;
 * a key >= n_world counts 0); both landmarks of a merged match count, their sum saturating at 2^32 - 1 (sums that reach it are
 * equal and keep their feature order).  The sort runs on the device, in the kernel that
 * builds the list (a stable LSD radix sort in LDS); with d_obs_counts == NULL this is hm_landmark_matches_batch_device.
 * Pass the lists to rs_p3p_arrsac_batch_device WITHOUT RS_BATCH_SHUFFLE to keep the order. */
int32_t hm_landmark_matches_ordered_batch_device(hm_ctx* ctx, const void* d_best, const void* d_decision, const void* d_merge_ok,
                                                 const void* d_obs_counts, const void* d_nq, const uint32_t* iq, uint32_t cap_per_img,
                                                 uint32_t n_frames, const void* d_world, uint32_t n_world, void* d_pairs,
                                                 void* d_npairs, void* stream_to_wait);
/* original_matches itself (cv-sfm/src/lib.rs:1549-1576), for rs_refine_poses_batch_device: the same lists in the same order
 * WITHOUT the drop of the matches whose triangulation is None — final_matches (lib.rs:1742-1758) needs them.  The arguments
 * of hm_landmark_matches_ordered_batch_device without the world table; n_world still numbers the rows (a merged match is row
 * n_world + f * cap + j, and a unique match on a landmark key >= n_world names no landmark of the table and is left out as
 * before).  Given a world table without "None" rows the entry point above writes the same bytes. */
int32_t hm_landmark_original_matches_batch_device(hm_ctx* ctx, const void* d_best, const void* d_decision, const void* d_merge_ok,
                                                  const void* d_obs_counts, const void* d_nq, const uint32_t* iq, uint32_t cap_per_img,
                                                  uint32_t n_frames, uint32_t n_world, void* d_pairs, void* d_npairs,
                                                  void* stream_to_wait);
/* hm_landmark_matches_batch_device without a merge mask (equals the reference when no decision-2 match passes the graph test). */
int32_t hm_landmark_pairs_batch_device(hm_ctx* ctx, const void* d_best, const void* d_decision, const void* d_nq, const uint32_t* iq,
                                       uint32_t cap_per_img, uint32_t n_frames, const void* d_world, uint32_t n_world,
                                       void* d_pairs, void* d_npairs, void* stream_to_wait);
/* matching()/symmetric_matching() of tutorial ch5 main.rs:154-200 and cv-sfm/src/lib.rs:3097-3133,
 * and match_descriptors() of akaze/tests/estimate_pose.rs:78-97.
 *   rule 0: accept iff d0 + param_u <  d1   (tutorial, param_u = 24)
 *   rule 1: accept iff d0 + param_u <= d1   (cv-sfm better_by = 24); returns no matches when either
 *           side has fewer than 2 descriptors (cv-sfm/src/lib.rs:3099-3101)
 *   rule 2: accept iff (f32)d0 < (f32)d1 * param_f   (Lowe ratio, estimate_pose.rs:91-93)
 * symmetric != 0 keeps [a,b] only when the reverse match of b is a.  pairs = [a0,b0,a1,b1,...],
 * ascending a. */
enum { HM_RULE_BETTER_BY_STRICT = 0, HM_RULE_BETTER_BY = 1, HM_RULE_LOWE = 2 };
int32_t hm_match(hm_ctx* ctx, const akz_descriptor* a, uint32_t na, const akz_descriptor* b,
                 uint32_t nb, int32_t rule, uint32_t param_u, float param_f, int32_t symmetric,
                 uint32_t* pairs, uint32_t cap, uint32_t* n_out);
/* Device-resident batched form: `n_pairs` independent (a,b) problems.  d_a/d_b are frame-major
 * descriptor blocks of cap_per_img entries each; d_na/d_nb the per-frame counts (device).
 * Problem p matches block ia[p] of d_a against block ib[p] of d_b (host index arrays).
 * d_pairs holds n_pairs*cap_per_img [a,b] pairs; d_n_out n_pairs counts.  Enqueued on the hm
 * context's stream after `stream_to_wait`. */
int32_t hm_match_batch_device(hm_ctx* ctx, const void* d_a, const void* d_na, const void* d_b,
                              const void* d_nb, uint32_t cap_per_img, const uint32_t* ia,
                              const uint32_t* ib, uint32_t n_pairs, int32_t rule, uint32_t param_u,
                              float param_f, int32_t symmetric, void* d_pairs, void* d_n_out,
                              void* stream_to_wait);
int32_t hm_sync(hm_ctx* ctx);

/* ---- frame-level place recognition ----
 * HammingHasher<64, 512>::hash_bag (cv-sfm/src/lib.rs:672; hasher built from the 4096-word codebook at :216):
 * every feature sets the hash bit of its nearest codeword (lowest index among equal distances), bit w at byte
 * w >> 3, position w & 7.  hash = n_codewords / 8 bytes (n_codewords a multiple of 32); words[i] (optional) =
 * {nearest codeword, distance} of feature i.  The hashing crate (hamming-lsh 0.3.2) is not vendored in the
 * reference: parity unpinned (oracle/lsh_oracle.c). */
int32_t hm_hash_bag(hm_ctx* ctx, const akz_descriptor* feats, uint32_t n, const akz_descriptor* codewords,
                    uint32_t n_codewords, uint8_t* hash, akz_neighbor* words);
/* Batched device-resident form: frame f = d_descs block f ([cap_per_img][64]) with count d_counts[f];
 * d_codewords [n_codewords][64]; d_hash [n_frames][n_codewords / 8]; d_words [n_frames][cap_per_img] of
 * akz_neighbor, required: it is the pass's intermediate.  Stream-ordered after stream_to_wait on hm_stream(). */
int32_t hm_hash_bag_device(hm_ctx* ctx, const void* d_descs, const void* d_counts, uint32_t cap_per_img,
                           uint32_t n_frames, const void* d_codewords, uint32_t n_codewords, void* d_hash,
                           void* d_words, void* stream_to_wait);
/* lsh_to_frame.knn_values(&lsh, k) (cv-sfm/src/lib.rs:622-624) as an exact search: the min(k, n) stored hashes
 * nearest to `query`, ascending (distance, index); hash_bytes a multiple of 4 (512 in cv-sfm). */
int32_t hm_hash_knn(hm_ctx* ctx, const uint8_t* query, const uint8_t* hashes, uint32_t n, uint32_t hash_bytes,
                    uint32_t k, akz_neighbor* out, uint32_t* n_out);
/* ---- which frames a frame is compared with, on the device ----
 * VSlamData::find_visually_similar_and_recent_frames (cv-sfm/src/lib.rs:597-668) and the order try_localize gives its
 * reconstructions (:853-855), for a batch of queries over a frame table that lives in the caller's device memory; add_frame
 * (:790-806) and try_localize_and_incorporate (:926-939) are the reference's callers.  Row i of the table is frame i in
 * insertion order: d_hashes [n_stored][hash_bytes] u8 the frame's lsh (hash_bytes a multiple of 4, <= HM_PL_MAX_HASH_BYTES; 512 in
 * cv-sfm — hm_hash_bag_device writes rows where it is told, so appending is pointing its d_hash at the table's tail), d_feed /
 * d_pos [n_stored] u32 Frame::feed / feed_frame, d_recon / d_view [n_stored] u32 the reconstruction and view key of Frame::view,
 * d_recon HM_PL_NONE for None (d_view is not read there).
 * Query q is about the stored row d_query[q] and sees the rows i < d_visible[q] (d_visible NULL: all n_stored; add_frame inserts
 * the frame and then asks: visible = query + 1).  In the reference's order:
 *   recent   the visible frames r != query of the query's feed with |pos[r] - pos[query]| < num_recent, ascending pos (:611-621);
 *            (feed, pos) is unique in a well-formed table: a second visible frame on one slot of the window is HM_PL_BAD_TABLE;
 *   search   the min(search_num, visible) visible hashes nearest to the query's, ascending (distance, row) over all bits, the
 *            query's own row like any other — exact where the reference asks an approximate index, hm_hash_knn's statement;
 *   similar  the search list in order without the query, without the recent frames and without the frames of the query's feed
 *            with |pos difference| < recent_threshold, then the first num_similar (:626-637);
 *   chain    recent then similar (:643): an entry with a view goes to its reconstruction's list, any other to the free list;
 *   groups   reconstructions by descending number of views found (:853-855), equal counts by ascending reconstruction key (the
 *            reference leaves those to a HashMap and an unstable sort).
 * Outputs, rows of pitch `room` >= hm_place_room(params) = max(2 * num_recent - 2, 0) + num_similar, entries past a count NOT
 * written: d_found [nq][room] the chain (stored rows); d_views_out [nq][room] the view keys, groups back to back in group order;
 * d_group_recon [nq][room] and d_group_start [nq][room + 1] (n_groups + 1 words written); d_free [nq][room]; d_search
 * [nq][search_num] akz_neighbor, optional: the search list; d_counts [nq][HM_PL_COUNTS] {n_recent, n_similar, n_searched,
 * n_groups, n_free}; d_verdict [nq] HM_PL_OK, HM_PL_BAD_INDEX (query >= n_stored, visible > n_stored or query >= visible) or
 * HM_PL_BAD_TABLE — on either refusal the query's counts are 0, nothing else of its rows is written and nothing was read through
 * the bad index.  nq <= 65535, search_num <= HM_PL_MAX_SEARCH, num_similar <= search_num, num_recent <= HM_PL_MAX_RECENT
 * (AKZ_E_INVALID / AKZ_E_TOO_LARGE, before the context is looked at).  Enqueued on hm_stream() after stream_to_wait; scratch
 * from the context; no host synchronisation and no readback.  With num_similar == 0 and d_search NULL the search is left out. */
typedef struct hm_place_params {
    uint32_t num_similar;        /* similar_frames: 0 (settings.rs:437-451) */
    uint32_t num_recent;         /* tracking_recent_frames: 32 */
    uint32_t recent_threshold;   /* similar_recent_threshold: 0 */
    uint32_t search_num;         /* similar_frames_search_num: 512 */
} hm_place_params;
enum { HM_PL_OK = 0, HM_PL_BAD_INDEX = 1, HM_PL_BAD_TABLE = 2 };
enum { HM_PL_C_RECENT = 0, HM_PL_C_SIMILAR = 1, HM_PL_C_SEARCHED = 2, HM_PL_C_GROUPS = 3, HM_PL_C_FREE = 4, HM_PL_COUNTS = 5 };
enum { HM_PL_MAX_HASH_BYTES = 4096, HM_PL_MAX_SEARCH = 2048, HM_PL_MAX_RECENT = 256 };
#define HM_PL_NONE 0xFFFFFFFFu
int32_t hm_place_params_default(hm_place_params* params);
uint32_t hm_place_room(const hm_place_params* params);
int32_t hm_find_frames_batch_device(hm_ctx* ctx, const void* d_hashes, const void* d_feed, const void* d_pos, const void* d_recon,
                                    const void* d_view, uint32_t n_stored, uint32_t hash_bytes, const void* d_query,
                                    const void* d_visible, uint32_t nq, const hm_place_params* params, uint32_t room, void* d_found,
                                    void* d_views_out, void* d_group_recon, void* d_group_start, void* d_free, void* d_search,
                                    void* d_counts, void* d_verdict, void* stream_to_wait);
/* The frame table behind rs_repack_table_device, in place: for the rows whose d_recon is `recon` (not HM_PL_NONE), d_view
 * becomes d_block_map[view] (NULL: the identity), and a removed view (0xFFFFFFFF) makes d_recon HM_PL_NONE — remove_view's
 * frame.view = None (cv-sfm/src/lib.rs:519); such a frame appears in d_free from then on.  A view >= n_blocks leaves its row
 * untouched and sets d_flags [1] u32 to 1 (0 otherwise).  Elementwise, one launch on hm_stream() after stream_to_wait. */
int32_t hm_place_remap_views_device(hm_ctx* ctx, void* d_recon, void* d_view, uint32_t n_stored, uint32_t recon, const void* d_block_map,
                                    uint32_t n_blocks, void* d_flags, void* stream_to_wait);
/* From the frames found to the searches, without a host step (cv_amd/csrc/hm_view_plan.hip; the decisions:
 * include/akz_view_plan_math.h).  The reference hands register_frame_subset the views of ONE reconstruction at a time
 * (try_localize, cv-sfm/src/lib.rs:858-891: a turn of its loop per group, most views found first; try_localize_and_incorporate,
 * :926-939: the group of one named reconstruction, .remove(&reconstruction)), and :1472-1486 walk exactly that list.
 *
 * hm_view_plan_device: frame f reads row f of an hm_find_frames_batch_device call's d_views_out, d_group_recon, d_group_start,
 * d_counts and d_verdict (pitch `room`, any room).  Its group: d_pick NULL -> group 0; d_pick [n_frames] u32 without
 * HM_VP_PICK_RECON in `flags` -> the ordinal d_pick[f]; with it -> the group whose d_group_recon equals d_pick[f].  Its list: the
 * first min(n_views, group length) view keys of that group in the group's order; a view key is a block of the descriptor table
 * (FrameIndex.set_views, hm_place_remap_views_device).  d_view_idx [n_frames][n_views] u32: the list, HM_PL_NONE at and behind
 * its length; d_n_views [n_frames]: the length; d_plan_verdict [n_frames]: HM_VP_OK, HM_VP_CUT (the group was longer than
 * n_views: still n_views of it), HM_VP_NO_GROUP (no such group, or none at all), HM_VP_FIND_REFUSED (the find's verdict is not
 * HM_PL_OK: none of its rows is read) or HM_VP_BAD_VIEW (a taken key >= n_blocks: the frame is refused alone and nothing is read
 * through the key) — length 0 for the last three.  d_plan_counts [HM_VP_COUNTS] u32 {distinct target blocks of all accepted
 * frames, live problems = the sum of the lengths, the call's verdict, frames with at least one view}: more distinct blocks
 * than exp_blocks is HM_VP_NO_ROOM — every frame's length is then 0 and its list HM_PL_NONE, so that a search planned from it
 * searches nothing; the frames keep their own verdicts.  n_views 1..HM_VP_MAX_VIEWS, exp_blocks >= 1, n_frames * n_views <= 65535,
 * n_frames + exp_blocks <= 65535 (AKZ_E_INVALID otherwise, before the context is looked at); n_frames 0: nothing to do.
 *
 * hm_knn_planned_batch_device: hm_knn_batch_device for the problems (f, v) = every feature of query block iq[f] (host list, the
 * new frames' blocks) of d_q against block d_view_idx[f][v] of d_t, for v < min(d_n_views[f], n_views) — lists that
 * hm_view_plan_device or any other kernel wrote.  d_out [n_frames][n_views][cap][k]; a live problem's slab holds the bytes
 * hm_knn_batch_device writes for it; the slab of a dead problem (v at or behind the frame's length, or a key >= n_blocks) is not
 * written.  The distinct target blocks are counted and ranked on the device and the recoding plan is written there: a job per
 * frame's query block and per distinct target block in ascending block order, so that no byte depends on arrival order.  The
 * grids come from the rooms alone — exp_blocks is the room for distinct target blocks — and no count is read back.  A list with
 * MORE distinct blocks than exp_blocks searches NOTHING: no slab is written.  hm_view_plan_device with the same exp_blocks has
 * then emptied every list (HM_VP_NO_ROOM); a caller with lists of its own makes exp_blocks min(n_frames * n_views, n_blocks).
 * cap_per_img and k as hm_knn_batch_device; the other limits as above.
 *
 * hm_best_of_views_planned_batch_device: hm_best_of_views_batch_device over those lists: frame f reads its first
 * min(d_n_views[f], n_views) slabs; a frame of length 0 gets {HM_PL_NONE, HM_PL_NONE} x 3 and decision 0 for each of its features.
 * A key >= n_blocks and a neighbour index at or behind its view's count are passed over.
 *
 * All three are stream-ordered on hm_stream() behind stream_to_wait, return after enqueueing and take their scratch from the
 * context. */
enum { HM_VP_OK = 0, HM_VP_CUT = 1, HM_VP_NO_GROUP = 2, HM_VP_FIND_REFUSED = 3, HM_VP_BAD_VIEW = 4, HM_VP_NO_ROOM = 5 };
enum { HM_VP_C_BLOCKS = 0, HM_VP_C_LIVE = 1, HM_VP_C_VERDICT = 2, HM_VP_C_FRAMES = 3, HM_VP_COUNTS = 4 };
enum { HM_VP_PICK_RECON = 1 };
enum { HM_VP_MAX_VIEWS = 64 };
int32_t hm_view_plan_device(hm_ctx* ctx, const void* d_views_out, const void* d_group_recon, const void* d_group_start, const void* d_counts,
                            const void* d_verdict, uint32_t room, const void* d_pick, uint32_t flags, uint32_t n_frames, uint32_t n_views,
                            uint32_t n_blocks, uint32_t exp_blocks, void* d_view_idx, void* d_n_views, void* d_plan_verdict, void* d_plan_counts,
                            void* stream_to_wait);
int32_t hm_knn_planned_batch_device(hm_ctx* ctx, const void* d_q, const void* d_nq, const void* d_t, const void* d_nt, uint32_t cap_per_img,
                                    const uint32_t* iq, const void* d_view_idx, const void* d_n_views, uint32_t n_frames, uint32_t n_views,
                                    uint32_t n_blocks, uint32_t exp_blocks, uint32_t k, void* d_out, void* stream_to_wait);
int32_t hm_best_of_views_planned_batch_device(hm_ctx* ctx, const void* d_knn, const void* d_nq, const uint32_t* iq, uint32_t cap_per_img,
                                              const void* d_view_idx, const void* d_n_views, uint32_t n_frames, uint32_t n_views,
                                              uint32_t n_blocks, uint32_t k, const void* d_landmarks, const void* d_nviews, uint32_t better_by,
                                              void* d_best, void* d_decision, void* stream_to_wait);
/* Optional timing of the k-NN kernel launches with HIP events on hm_stream() (bench.py's matcher roofline):
 * hm_timing_get waits for the pending events and returns the accumulated milliseconds / launch count.  A symmetric match
 * whose reverse side is answered from the forward lists counts as ONE launch, and its decision and verification kernels and
 * the skippable reverse search add their time to it: an operation count divided by this time is an equivalent brute-force
 * rate.  (The VALU switch times nothing of a match.) */
int32_t hm_timing_enable(hm_ctx* ctx, int32_t on);
int32_t hm_timing_get(hm_ctx* ctx, double* ms, uint64_t* launches, int32_t reset);
void* hm_stream(hm_ctx* ctx);

/* ---- two-view geometric verification (second phase) ---- */
typedef struct rs_ctx rs_ctx;
/* The context's stream (rs_stream) is created at the MOST urgent priority of the device: a consensus is a chain of hundreds
 * of small dependent launches, and behind bulk kernels of equal priority (a matcher, an extraction) every one of them queues
 * for compute units — the registration loop of bench.py ran 142.6 -> 126.5 ms per 256 frames on that change alone. */
int32_t rs_create(int32_t device, uint32_t max_matches, uint32_t max_hypotheses, rs_ctx** out);
int32_t rs_destroy(rs_ctx* ctx);
/* cv_pinhole::CameraIntrinsics::calibrate (cv-pinhole/src/lib.rs:108-117) and, with use_k1 != 0,
 * CameraIntrinsicsK1Distortion::calibrate (:191-202): pixel keypoints -> unit bearings [n][3].
 * intrinsics = {focal_x, focal_y, principal_x, principal_y, skew}.  Host-only scalar math. */
int32_t rs_calibrate(const double* intrinsics, int32_t use_k1, double k1, const akz_keypoint* kps, uint32_t n,
                     double* bearings);
/* Consensus::model_inliers(&EightPoint::new(), matches) (call sites akaze/tests/estimate_pose.rs:63-67,
 * tutorial ch5 main.rs:70-72, cv-sfm/src/lib.rs:1394-1406) with the sampler factored out: the caller
 * provides n_hyp minimal samples (8 match indices each, what arrsac draws from its RNG); every sample is
 * turned into an essential matrix (eight-point/src/lib.rs:43-58) and its four poses
 * (cv-pinhole/src/essential.rs:217-231), every pose is scored against all n matches with
 * CameraToCamera::residual (cv-core/src/pose.rs:249-295) < thresh, and the pose with the most inliers wins
 * (ties: lowest hypothesis, then lowest pose index).  best_pose = row-major 3x4 [R | t];
 * best_id = hypothesis*4 + pose, 0xFFFFFFFF if no sample produced a model (the reference returns None);
 * inlier_idx ascending. */
int32_t rs_essential_batch(rs_ctx* ctx, const double* bearings_a, const double* bearings_b, uint32_t n,
                           const uint32_t* sample_idx, uint32_t n_hyp, double thresh, double* best_pose,
                           uint32_t* best_id, uint32_t* inlier_idx, uint32_t cap, uint32_t* n_inliers);
/* Consensus::model_inliers(&NisterStewenius::new(), matches): the same with the five-point minimal solver for calibrated
 * cameras (nister-stewenius/src/lib.rs:50-330).  sample_idx [n_samples][5]; a sample has up to ten essential matrices
 * (include/akz_five_point_math.h: the reference's algorithm with rows 6..9 of the action matrix's eigenvector — rows 5..8 as
 * written at lib.rs:230 do not solve the problem), in ascending order of the action matrix's eigenvalue;
 * sample h owns the hypothesis slots 10 h .. 10 h + 9, unused ones hold no model, and each solution goes through the
 * eight-point path's E -> four poses -> residual.  best_id = (10 sample + solution) 4 + pose.  The context needs
 * 10 x n_samples hypothesis slots (rs_create's max_hypotheses), else AKZ_E_INVALID; n < 5 gives no model
 * (best_id 0xFFFFFFFF, AKZ_OK). */
int32_t rs_five_point_batch(rs_ctx* ctx, const double* bearings_a, const double* bearings_b, uint32_t n,
                            const uint32_t* sample_idx, uint32_t n_samples, double thresh, double* best_pose,
                            uint32_t* best_id, uint32_t* inlier_idx, uint32_t cap, uint32_t* n_inliers);
/* The same consensus in arrsac's shape (arrsac::Arrsac::model_inliers; parameters as its builder exposes them at
 * vslam-sandbox/src/main.rs:105-117: initialization_hypotheses, max_candidate_hypotheses, block_size,
 * likelihood_ratio_threshold): the hypotheses are scored breadth-first, `block_size` matches at a time, and after
 * every block a pose is retired when
 *   RS_PRUNE_BOUND  its count plus the matches still to come cannot reach the best count so far (exact: the winner,
 *                   its count and its inlier set equal exhaustive scoring's — rs_essential_batch on the same samples);
 *   max_candidates  it is not among the max_candidates best once init_blocks blocks have been scored (0 = no cap);
 *                   poses are ranked by their exact distance to the best count (distances of 2047 and more rank
 *                   together, after all others), equal ranks in ascending pose id: the best-supported poses are never
 *                   the ones the cap retires;
 *   RS_PRUNE_SPRT   Wald's sequential test rejects it: (delta/eps)^c ((1-delta)/(1-eps))^(seen-c) > sprt_ratio with
 *                   eps = best count / seen and delta = sprt_delta, the inlier rate expected of a wrong model;
 *   RS_PRUNE_HALVE  the candidate cap halves with every block after init_blocks (ARRSAC's preemption function
 *                   f(i) = floor(M 2^-floor(i/B))), down to one survivor; with estimations_per_block == 0 the block
 *                   loop ends when the cap reaches 1 (a single survivor cannot be overtaken; stats count what ran).
 * The rules in full (tests/consensus_statement.py states them in Python and holds oracle and device to that statement):
 *   blocks      With none of the rules asked for (no RS_PRUNE_BOUND, no RS_PRUNE_SPRT, max_candidates == 0,
 *               estimations_per_block == 0) all matches are one block.  Otherwise the decisions below are taken after every
 *               block but the last: nothing is retired and nothing re-sampled once every match has been scored.  `best` is
 *               the largest count among the live poses, `seen` the matches scored so far, `left` = n - seen.
 *   bound       count + left < best retires a pose.  It is applied wherever blocks are decided, also without RS_PRUNE_BOUND
 *               (it cannot change the result); the flag alone asks for block-wise scoring.
 *   SPRT        only while 0 < best < seen.  With natural logarithms from the host's libm the test is
 *               c l_in + (seen - c) l_out > ln(sprt_ratio), evaluated in this form in f64:
 *               l_in = ln(delta) - (ln(best) - ln(seen)),  l_out = ln(1 - delta) - (ln(seen - best) - ln(seen)).  Its left side is -seen KL(eps || delta)
 *               <= 0 at c == best, and it grows with c where eps <= delta: a pose at the best count is never rejected, and
 *               while eps <= delta no pose is (the implementations say both outright; neither changes a decision).
 *   cap         applies when more poses are live than the cap allows.  The ranking (distance to best, then id) is taken over
 *               the live poses as they entered this block's decisions.  Poses nearer than the cap-th of that ranking stay
 *               if bound and SPRT let them; the places the nearer ones leave go, in ascending id, to the poses as far as
 *               the cap-th one that bound and SPRT have not retired: a retired pose takes no place.
 *   halving     after block b >= init_blocks the cap is max(1, max_candidates >> (b - init_blocks)) (shifts of 31 and more
 *               give 1): with init_blocks == 0 the first decision, after block 1, already halves once.
 *   re-sampling after every block b >= init_blocks but the last: the best pose is the live one with the largest count, lowest
 *               id; its inliers among the matches seen are listed in scoring order; sample number h (numbers go on from
 *               n_hypotheses, estimations_per_block a round) draws K distinct positions of that list from stream h of
 *               seed ^ 0xA5A5A5A55A5A5A5A.  A round whose list is shorter than K, or that finds no live pose, draws
 *               nothing and still takes its numbers.  New poses are scored on the matches seen and join after the
 *               block's retirements.
 *   result      the live pose with the largest count over the matches scored, lowest id; inlier_idx lists its inliers among
 *               ALL matches in ascending index, also when the halving ended the loop early.
 *   stats       poses = 4 x the hypothesis slots numbered (rounds that drew nothing included); survivors = live poses at the
 *               end; blocks = blocks scored; residuals_evaluated = every (live pose, match) of every block, + seen for the
 *               list of a re-sampling round that found a live pose, + seen for every valid pose it added (the final inlier
 *               list is not counted); residuals_exhaustive = poses x n.  A scene of a batched call with fewer matches than
 *               a minimal sample has all of them zero.
 * n smaller than a minimal sample: AKZ_E_INVALID from the single-scene entries ("no model" for such a scene of a batched
 * call).  "No model" otherwise means that no sample gave a pose.  The eight-point solver gives four poses for ANY eight
 * matches, also for one match repeated eight times (it takes a vector of the then eight-dimensional null space): such a
 * call returns a pose without support, best_id 0 and an empty inlier list, not "no model".  Lambda Twist on three equal
 * points gives none.
 * sample_idx == NULL draws the n_hypotheses minimal samples on the device from xoshiro256++ streams seeded with
 * `seed` (rs_arrsac_samples reproduces them on the host): stream h is xoshiro256++ whose four state words are the first four
 * outputs of splitmix64 started at seed + 0xD1B54A32D192ED03 (h + 1); an index is (next() >> 32) * n >> 32, a repeated
 * index is drawn again.  The arrsac crate is not vendored in the reference: the
 * sampler, the retirement rules and their order are this library's, specified by oracle/arrsac_oracle.c and held to
 * it bit for bit (parity with the crate unpinned beyond the count pin of akaze/tests/estimate_pose.rs:75).
 * best_id / best_pose / inlier_idx as for rs_essential_batch.
 *
 * RS_ESTIMATOR_FIVE_POINT (rs_essential_arrsac and rs_essential_arrsac_batch_device only; the P3P entry points refuse it):
 * the estimator is NisterStewenius instead of EightPoint.  n_hypotheses and estimations_per_block then count five-match
 * SAMPLES, each of which takes ten hypothesis slots of the context (see rs_five_point_batch; sample_idx is [n][5]);
 * max_candidates and stats.poses keep counting poses, best_id = (10 sample + solution) 4 + pose. */
enum { RS_PRUNE_BOUND = 1u << 0, RS_PRUNE_SPRT = 1u << 1, RS_PRUNE_HALVE = 1u << 2, RS_ESTIMATOR_FIVE_POINT = 1u << 3 };
typedef struct rs_arrsac_params {
    uint32_t struct_size;      /* sizeof(rs_arrsac_params) */
    uint32_t n_hypotheses;     /* initialization_hypotheses */
    uint32_t block_size;       /* matches per scoring block */
    uint32_t init_blocks;      /* blocks scored before max_candidates applies */
    uint32_t max_candidates;   /* max_candidate_hypotheses (poses kept); 0 = no cap */
    uint32_t flags;            /* RS_PRUNE_*, RS_ESTIMATOR_FIVE_POINT */
    double threshold;          /* inlier threshold on CameraToCamera::residual */
    double sprt_delta;         /* P(inlier | wrong model), e.g. 0.05 */
    double sprt_ratio;         /* likelihood ratio threshold, arrsac default 1e3 */
    uint64_t seed;             /* sampler seed (Xoshiro256PlusPlus::seed_from_u64 at the call sites) */
    uint32_t estimations_per_block; /* hypotheses generated after every block (from init_blocks on) from minimal samples
                                  * drawn among the inliers of the best pose so far — arrsac's inlier-guided
                                  * re-sampling; each is scored on all matches seen so far and joins the candidates;
                                  * 0 = off.  The context must hold n_hypotheses + this x blocks hypotheses. */
    uint32_t reserved;         /* must be zero */
} rs_arrsac_params;
typedef struct rs_arrsac_stats {
    uint32_t poses, survivors, blocks, reserved;
    uint64_t residuals_evaluated, residuals_exhaustive;
} rs_arrsac_stats;
int32_t rs_essential_arrsac(rs_ctx* ctx, const double* bearings_a, const double* bearings_b, uint32_t n,
                            const uint32_t* sample_idx, const rs_arrsac_params* params, double* best_pose,
                            uint32_t* best_id, uint32_t* inlier_idx, uint32_t cap, uint32_t* n_inliers,
                            rs_arrsac_stats* stats);
/* The same for Consensus::model_inliers(&LambdaTwist::new(), landmark matches) — the registration path's consensus
 * (cv-sfm/src/lib.rs:1619-1622; vslam-sandbox/src/main.rs:105-111: 16384 initialisation hypotheses, 1024 candidates):
 * 3-match samples, WorldToCamera::residual; bearings / world as for rs_p3p_batch. */
int32_t rs_p3p_arrsac(rs_ctx* ctx, const double* bearings, const double* world, uint32_t n,
                      const uint32_t* sample_idx, const rs_arrsac_params* params, double* best_pose,
                      uint32_t* best_id, uint32_t* inlier_idx, uint32_t cap, uint32_t* n_inliers,
                      rs_arrsac_stats* stats);
/* The minimal samples the two functions draw on the device for (seed, n): sample_size 8 (eight-point), 5 (five-point) or
 * 3 (P3P). */
int32_t rs_arrsac_samples(uint64_t seed, uint32_t n, uint32_t n_hyp, uint32_t sample_size, uint32_t* sample_idx);
/* Consensus::model_inliers(&LambdaTwist::new(), matches) for 3D-2D registration (cv-sfm/src/lib.rs:1619-1622,
 * lambda-twist/tests/consensus.rs:59-61), sampler factored out as above: n_hyp sample triples; each gives up
 * to four WorldToCamera poses (lambda-twist/src/lib.rs:107-318), scored with WorldToCamera::residual
 * (cv-core/src/pose.rs:194-201) < thresh.  bearings [n][3] unit vectors, world [n][4] homogeneous points in the
 * reference's Projective form (xyz normalised, w = 1/distance). */
int32_t rs_p3p_batch(rs_ctx* ctx, const double* bearings, const double* world, uint32_t n,
                     const uint32_t* sample_idx, uint32_t n_hyp, double thresh, double* best_pose,
                     uint32_t* best_id, uint32_t* inlier_idx, uint32_t cap, uint32_t* n_inliers);
/* parity tap: inlier counts [n_hyp][4] of the last rs_essential_batch / rs_p3p_batch call */
int32_t rs_debug_counts(rs_ctx* ctx, uint32_t* counts, uint32_t cap);
/* parity tap: poses [n_hyp][4][12] (row-major [R | t]) and validity flags [n_hyp][4] of the last single-scene call —
 * what EightPoint::estimate / LambdaTwist::estimate returned for each minimal sample (eight-point/src/lib.rs:70-83,
 * lambda-twist/src/lib.rs:330-347) */
int32_t rs_debug_poses(rs_ctx* ctx, double* poses, uint32_t* ok, uint32_t n_hyp);
/* parity tap: the essential matrices E [n_samples][10][9] (row-major, b^T E a = 0; slots beyond a sample's count are
 * zero-filled) and the solution counts [n_samples] of the last single-scene five-point call (rs_five_point_batch, or
 * rs_essential_arrsac with RS_ESTIMATOR_FIVE_POINT).  rs_debug_poses / rs_debug_counts see n_hyp = 10 x n_samples.
 * Any other consensus call on the context since — another estimator, or a batched device entry — leaves nothing to read:
 * AKZ_E_INVALID for n_samples >= 1. */
int32_t rs_debug_essentials(rs_ctx* ctx, double* E, uint32_t* n_solutions, uint32_t n_samples);

/* parity tap: CameraToCamera::residual (cv-core/src/pose.rs:249-295) of every (pose, match) as the device evaluates it.
 * poses [n_pose][12] row-major [R | t], bearings [n][3], host buffers.  paired == 0: out [n_pose][n].  paired != 0: out
 * [n_pose][2][n] — the pose and its mirror image [R | -t] (poses p and p + 2 of a hypothesis) through the path that
 * shares one eigen-decomposition between the two. */
int32_t rs_debug_residuals(rs_ctx* ctx, const double* poses, uint32_t n_pose, const double* bearings_a, const double* bearings_b,
                           uint32_t n, int32_t paired, double* out);
/* parity tap of the shortcut in front of the eigen-decomposition (rs_pair_far): out[pose * n + match] = 1 where
 * the epipolar-plane bound alone proves residual >= thresh for [R | t] and [R | -t]; tests hold it to rs_debug_residuals. */
int32_t rs_debug_far(rs_ctx* ctx, const double* poses, uint32_t n_pose, const double* bearings_a, const double* bearings_b,
                     uint32_t n, double thresh, uint8_t* out);

/* ---- two-view verification of a whole micro-batch, device-resident ----
 * What cv-sfm does for every frame pair the matcher produced (cv-sfm/src/lib.rs:1385-1412): shuffle the matches,
 * map them to calibrated bearing pairs (match_ix_kps; CameraIntrinsics::calibrate, cv-pinhole/src/lib.rs:108-117),
 * run the consensus (vslam-sandbox/src/main.rs:112-117: Arrsac, 8192 initialisation hypotheses, 1024 candidates),
 * keep the inliers.  Here all frame pairs of a micro-batch go through ONE chain of launches (grid = scenes x
 * hypotheses), reading the matcher's pair lists and the extractor's keypoints where they lie in HBM.
 *
 * rs_camera: CameraIntrinsics {focals, principal_point, skew} and, with use_k1 != 0, CameraIntrinsicsK1Distortion's k1. */
typedef struct rs_camera {
    double fx, fy, cx, cy, skew;
    double k1;
    int32_t use_k1;
    int32_t reserved;   /* must be zero */
} rs_camera;
/* Room for up to max_scenes frame pairs per call (rs_create leaves room for one); every scene gets the context's
 * max_matches matches and max_hypotheses hypotheses.  1 <= max_scenes <= 65535. */
int32_t rs_batch_reserve(rs_ctx* ctx, uint32_t max_scenes);
enum { RS_BATCH_SHUFFLE = 1u << 0 };   /* score the matches in a seeded shuffled order (the reference shuffles them with
                                        * the caller's rng, cv-sfm/src/lib.rs:1385): position j of scene s holds the
                                        * match with the j-th smallest 32-bit key splitmix64((seed_s ^ 0x5851F42D4C957F2D)
                                        * + 0xD1342543DE82EF95 j) >> 32 (splitmix64(x): the first output of the generator
                                        * started at x, i.e. the mix of x + 0x9E3779B97F4A7C15), ties in index order; needs
                                        * cap_per_img <= 8192 */
/* Scene s (0 <= s < n_scenes): pair list s of d_pairs ([cap_per_img][2] u32, count d_npairs[s] — hm_match_batch_device's
 * outputs), whose [a, b] index the keypoints of block ia[s] of d_kps_a and block ib[s] of d_kps_b ([..][cap_per_img]
 * akz_keypoint — akz_extract_batch_device's output).  Each scene runs rs_essential_arrsac's procedure on its calibrated
 * bearing pairs with the sampler seed  params->seed + 0x9E3779B97F4A7C15 * s  (scene 0 = the caller's seed; match
 * counts above max_matches are clipped).  Outputs, device arrays indexed by scene: d_pose [12] f64 row-major [R | t],
 * d_best_id u32 (0xFFFFFFFF: no model — fewer than 8 matches, or no sample produced one), d_inliers [cap_per_img] u32
 * (ascending indices into the scene's pair list), d_n_inliers u32, d_stats (optional) rs_arrsac_stats.  Enqueued on
 * rs_stream() after stream_to_wait (may be NULL); returns after enqueueing, rs_sync() waits.  Specified by
 * oracle/arrsac_oracle.c (orc_arrsac_pairs) and held to it bit for bit. */
int32_t rs_essential_arrsac_batch_device(rs_ctx* ctx, const void* d_kps_a, const void* d_kps_b, uint32_t cap_per_img,
                                         const uint32_t* ia, const uint32_t* ib, const void* d_pairs, const void* d_npairs,
                                         uint32_t n_scenes, const rs_camera* cam_a, const rs_camera* cam_b,
                                         const rs_arrsac_params* params, uint32_t flags, void* d_pose, void* d_best_id,
                                         void* d_inliers, void* d_n_inliers, void* d_stats, void* stream_to_wait);
/* The registration path's consensus for a micro-batch of new frames (cv-sfm/src/lib.rs:1571-1622: FeatureWorldMatch(bearing,
 * point) list -> single_view_consensus.model_inliers(&LambdaTwist, ..)).  Scene s: pair list s of d_pairs ([cap_per_img][2]
 * u32, count d_npairs[s]) whose entries are {feature index into keypoint block ik[s] of d_kps, index into d_world};
 * d_world [n_world][4] f64 homogeneous world points (the triangulated landmarks: rs_triangulate_landmarks_device).  A scene whose pair list names a
 * feature >= cap_per_img or a world point >= n_world is refused as a whole (no model; nothing is read out of bounds); the
 * two-view entry point above treats a pair that points outside its keypoint blocks the same way.   bearing = calibrate(keypoint); each
 * scene runs rs_p3p_arrsac's procedure with the scene seed as above.  Outputs as above (pose = WorldToCamera [R | t];
 * no model: fewer than 3 matches or no sample produced a pose).  Specified by oracle/arrsac_oracle.c (orc_p3p_arrsac_pairs). */
int32_t rs_p3p_arrsac_batch_device(rs_ctx* ctx, const void* d_kps, uint32_t cap_per_img, const uint32_t* ik, const void* d_pairs,
                                   const void* d_npairs, uint32_t n_scenes, const void* d_world, uint32_t n_world,
                                   const rs_camera* cam, const rs_arrsac_params* params, uint32_t flags, void* d_pose,
                                   void* d_best_id, void* d_inliers, void* d_n_inliers, void* d_stats, void* stream_to_wait);

/* ---- triangulation on the device: the world table of the registration chain, the points of a two-view consensus ----
 * cv-geom's LinearEigenTriangulator::triangulate_observations (cv-geom/src/triangulation.rs:82-130) — one 4 x 4 symmetric
 * eigen-problem per point — and around it cv-sfm's triangulate_landmark_robust / triangulate_merged_landmark_robust
 * (cv-sfm/src/lib.rs:2895-3000).  The arithmetic is include/akz_triangulate_math.h (compiled for the device and, by the
 * tests, for the host: equal bit for bit); nalgebra's eigen-solver and product order and the order of a landmark's
 * observations (a HashMap in the reference, the caller's list here) are unpinned.
 * "None" is written as the row {0, 0, 0, -1} — the w < 0 the registration chain reads as "no robust triangulation" — and,
 * where a reason array is given, one byte per row says why: */
enum {
    RS_TRI_OK = 0, RS_TRI_TOO_FEW = 1 /* fewer than 2 observations */, RS_TRI_NOT_ROBUST = 2, RS_TRI_EIGEN = 3 /* the solver
    did not converge within max_sweeps */, RS_TRI_NOT_FINITE = 4, RS_TRI_CHEIRALITY = 5 /* behind an observing camera */,
    RS_TRI_BAD_INDEX = 6 /* an observation or a list names something outside the caller's arrays: nothing is read out of bounds */
};
enum { RS_TRI_MAX_SWEEPS = 1024 };   /* sweeps the device runs at the most, whatever max_sweeps says (a 4 x 4 problem needs < 20) */
typedef struct rs_triangulate_params {
    uint32_t struct_size;                       /* sizeof(rs_triangulate_params) */
    uint32_t max_sweeps;                        /* LinearEigenTriangulator::max_iterations (1000), >= 1: sweeps of the cyclic Jacobi
                                                 * iteration, as the residual path passes to akz_rm_jacobi4_sym; values above
                                                 * RS_TRI_MAX_SWEEPS count as RS_TRI_MAX_SWEEPS */
    double eps;                                 /* LinearEigenTriangulator::epsilon, default 1e-12 */
    uint32_t robust_minimum_observations;       /* cv-sfm/src/settings.rs:344-350: 3 */
    uint32_t n_views;                           /* views of the reconstruction, for the min() of lib.rs:2913-2917 */
    double incidence_minimum_cosine_distance;   /* 1e-3 */
} rs_triangulate_params;
/* the reference's defaults; n_views = 0xFFFFFFFF (the min() then is robust_minimum_observations) */
int32_t rs_triangulate_params_default(rs_triangulate_params* params);
/* triangulate_observations for ONE list: poses [n][12] row-major [R | t] WorldToCamera, bearings [n][3] unit vectors — host
 * buffers in and out, computed on the device; the robustness test is NOT applied.  point [4], reason (optional) one byte.
 * A convenience for single lists: every call allocates, copies, launches one lane and waits.  A loop over the inliers of a
 * consensus belongs on rs_triangulate_pairs_batch_device, a loop over landmarks on rs_triangulate_landmarks_device. */
int32_t rs_triangulate_observations(rs_ctx* ctx, const double* poses, const double* bearings, uint32_t n,
                                    const rs_triangulate_params* params, double* point, uint8_t* reason);
/* The world table: row l of d_world ([>= n_landmarks][4] f64) = triangulate_landmark_robust(landmark l) for every l <
 * n_landmarks.  Landmark l's observations are entries d_obs_start[l] .. d_obs_start[l + 1] (d_obs_start [n_landmarks + 1]
 * u32, ascending) of d_obs ([n_obs][2] u32 {block, feature}), in that order; observation {b, j} = the calibrated bearing of
 * keypoint j of block b of d_kps ([n_blocks][cap_per_img] akz_keypoint, akz_extract_batch_device's output) under the pose
 * d_poses[b] ([n_blocks][12] f64 WorldToCamera).  A list that names a block >= n_blocks or a feature >= cap_per_img, or
 * whose range leaves [0, n_obs], gives reason 6 for that landmark.  d_reason (optional) [n_landmarks] u8.  One launch on
 * rs_stream() after stream_to_wait (may be NULL); returns after enqueueing. */
int32_t rs_triangulate_landmarks_device(rs_ctx* ctx, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks,
                                        const void* d_poses, const rs_camera* cam, const void* d_obs_start, const void* d_obs,
                                        uint32_t n_obs, uint32_t n_landmarks, const rs_triangulate_params* params, void* d_world,
                                        void* d_reason, void* stream_to_wait);
/* The rows of the merge candidates: for frame slot f < n_frames and feature j < cap_per_img with d_decision[f][j] == 2 and
 * d_merge_ok[f][j] != 0 (d_best [n_frames][cap][3] {landmark, distance} and d_decision [n_frames][cap] as
 * hm_best_of_views_batch_device leaves them, d_merge_ok [n_frames][cap] u8 the caller's are_landmarks_sharing_view verdicts)
 * row n_world + f * cap_per_img + j of d_world = triangulate_merged_landmark_robust([best0, best1]): the observations of
 * landmark d_best[f][j][0] followed by those of d_best[f][j][1], the robustness test on the concatenation
 * (cv-sfm/src/lib.rs:2958-2972).  No other row is written.  A landmark >= n_landmarks: reason 6.  d_reason (optional)
 * [n_frames][cap] u8, written where a row is. */
int32_t rs_triangulate_merged_device(rs_ctx* ctx, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses,
                                     const rs_camera* cam, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
                                     uint32_t n_landmarks, const rs_triangulate_params* params, const void* d_best,
                                     const void* d_decision, const void* d_merge_ok, uint32_t n_frames, uint32_t n_world,
                                     void* d_world, void* d_reason, void* stream_to_wait);
/* The CameraPoint of every inlier of a two-view consensus (cv-sfm/src/lib.rs:1023-1029, 1332: triangulate_relative(pose, a,
 * b) = triangulate_observations on (identity, a), (pose, b)), behind rs_essential_arrsac_batch_device with the same
 * keypoints, frame lists, pair lists and cameras and that call's outputs: scene s with a model (d_best_id[s] !=
 * 0xFFFFFFFF), inlier i < d_n_inliers[s]: d_points[s][i] ([n_scenes][cap_per_img][4] f64), d_reason (optional)
 * [n_scenes][cap_per_img] u8.  No robustness test on this path (the reference has none).  A scene without a model writes
 * nothing.  n_scenes within rs_batch_reserve's room (AKZ_E_TOO_LARGE beyond it).  ia / ib travel through the context's own
 * per-scene frame lists, the ones the consensus call filled: hand over the same lists. */
int32_t rs_triangulate_pairs_batch_device(rs_ctx* ctx, const void* d_kps_a, const void* d_kps_b, uint32_t cap_per_img,
                                          const uint32_t* ia, const uint32_t* ib, const void* d_pairs, const void* d_npairs,
                                          uint32_t n_scenes, const rs_camera* cam_a, const rs_camera* cam_b, const void* d_pose,
                                          const void* d_best_id, const void* d_inliers, const void* d_n_inliers,
                                          const rs_triangulate_params* params, void* d_points, void* d_reason, void* stream_to_wait);
/* ---- the three-view bootstrap of a reconstruction on the device ----
 * What cv-sfm's VSlam::init_reconstruction does for ONE combination of two two-view consensuses of a centre frame
 * (cv-sfm/src/lib.rs:1002-1300), for n_scenes combinations side by side: the depth ratios of the common matches and their
 * median as the scale of the second pose, the optimisation matches (the first three_view_optimization_landmarks that pass
 * is_tri_landmark_robust, in list order), the robust bearing pairs, three_view_filter_loop_iterations + 1 runs of
 * three_view_simple_optimize_l2 (cv-optimize/src/three_view_optimizer.rs:126-200) with the filter between them, and the
 * final masks and counts.  One persistent workgroup per triple, one launch.  The arithmetic is
 * include/akz_three_view_math.h (compiled for the device and, by the tests, for the host: equal bit for bit); its head
 * lists what is unpinned against the reference — nalgebra's from_scaled_axis, and the order of the sum over landmarks,
 * which is fixed there.  The HashMap join of the two pair lists and the shuffle (lib.rs:992-999, the caller's RNG in the
 * reference) are not this call's: rs_join_pairs_batch_device writes the lists it reads.
 * Verdicts.  The reference `continue`s to the next combination on every one of them but RS_TV_FEW_BEARING_PAIRS, where it
 * `return`s None: a caller that mirrors it ends its whole search there. */
enum {
    RS_TV_OK = 0,
    RS_TV_FEW_SCALES = 1,         /* fewer than three_view_minimum_relative_scales depth ratios (lib.rs:1039): continue */
    RS_TV_FEW_BEARING_PAIRS = 2,  /* fewer than robust_view_num_robust_bearing_pair (lib.rs:1100): return None */
    RS_TV_FEW_MATCHES = 3,        /* fewer than hard_minimum_matches entering a run (lib.rs:1118, 1167): continue */
    RS_TV_LOST_HALF = 4,          /* no more than half of the first optimisation matches left (lib.rs:1126, 1175, 1281): continue */
    RS_TV_FEW_ROBUST = 5,         /* num_robust_matches < three_view_minimum_robust_matches (lib.rs:1286): continue */
    RS_TV_BAD_INDEX = 6           /* a feature >= cap_per_img or a block >= n_blocks: the scene is refused, nothing read out of bounds */
};
enum {
    RS_TV_MAX_LANDMARKS = 1024,       /* three_view_optimization_landmarks at the most (they live in one workgroup's LDS) */
    RS_TV_MAX_RUNS = 9,               /* three_view_filter_loop_iterations + 1 at the most */
    RS_TV_MAX_ITERATIONS = 1 << 20,   /* a larger three_view_patience counts as this: the bound that ends every run */
    RS_TV_MAX_COMMON = 9216,          /* cap_per_img at the most (the depth ratios of the first pass wait in LDS for their median) */
    /* d_stats words (u32) of a scene: */
    RS_TV_S_SCALES = 0,               /* depth ratios found */
    RS_TV_S_MEDIAN = 1,               /* [2] median_scale (after the sqrt) as the bits of its f64, low word first */
    RS_TV_S_PAIRS = 3,                /* robust bearing pairs */
    RS_TV_S_RUN_MATCHES = 4,          /* [9] optimisation matches entering run r; 0xFFFFFFFF: not reached */
    RS_TV_S_RUN_STOP = 13,            /* [9] the iteration run r left its loop at (patience - 1: the last one; less: 50 iterations
                                       * without improvement); 0xFFFFFFFF: not run */
    RS_TV_S_ROBUST = 22,              /* num_robust_matches */
    RS_TV_S_STAGE = 23,               /* where the verdict fell: 0 indices, 1 scales, 2 bearing pairs, 3 + r entering run r, 12 the end */
    RS_TV_STATS = 24
};
typedef struct rs_three_view_params {
    uint32_t struct_size;                                         /* sizeof(rs_three_view_params) */
    uint32_t robust_view_num_robust_bearing_pair;                 /* 3 */
    double maximum_cosine_distance;                               /* 1e-5 */
    double maximum_sine_distance;                                 /* 1e-1 */
    double robust_observation_incidence_minimum_cosine_distance;  /* 1e-3 */
    double robust_view_bearing_pair_minimum_cosine_distance;      /* 1e-2 */
    double optimization_rate;                                     /* 0.001, the literal of lib.rs:1133 */
    uint32_t three_view_minimum_relative_scales;                  /* 16 */
    uint32_t three_view_filter_loop_iterations;                   /* 8; more than RS_TV_MAX_RUNS - 1: AKZ_E_INVALID */
    uint32_t three_view_optimization_landmarks;                   /* 1024; more than RS_TV_MAX_LANDMARKS: AKZ_E_TOO_LARGE */
    uint32_t three_view_patience;                                 /* 65536: the optimiser's iteration limit */
    uint32_t three_view_minimum_robust_matches;                   /* 32 */
    uint32_t hard_minimum_matches;                                /* 32, the literal of lib.rs:1118, 1167 */
    rs_triangulate_params triangulate;                            /* the eigen-solver's settings */
} rs_three_view_params;
/* the reference's defaults (cv-sfm/src/settings.rs:320-427) */
int32_t rs_three_view_params_default(rs_three_view_params* params);
/* Scene s: centre block ic[s], first i_first[s], second i_second[s] of d_kps ([n_blocks][cap_per_img] akz_keypoint as
 * akz_extract_batch_device leaves them; bearing = CameraIntrinsics::calibrate); d_pose_first / d_pose_second [n_scenes][12]
 * the CameraToCamera poses centre -> first / second as rs_essential_arrsac_batch_device writes them; d_triples
 * [n_scenes][cap_per_img][3] u32 {centre, first, second feature} the common matches in the caller's (shuffled) order,
 * d_ntriples [n_scenes]; d_first_only / d_second_only [n_scenes][cap_per_img][2] u32 {centre, other feature} the matches of
 * one pair whose centre feature the other pair does not have, with their counts.  Counts above cap_per_img count as it.
 * Outputs: d_verdict [n_scenes] u32 (RS_TV_*), d_stats [n_scenes][RS_TV_STATS] u32 — always written; and for RS_TV_OK only
 * d_pose_out [n_scenes][2][12] the optimised poses, d_combined [n_scenes][cap_per_img] u8 (lib.rs:1193-1210, one byte per
 * common match), d_first_ok / d_second_ok [n_scenes][cap_per_img] u8 (lib.rs:1212-1246) — a rejected scene's are left as
 * they were.  n_scenes within rs_batch_reserve's room (AKZ_E_TOO_LARGE beyond it).  The parameters are checked before
 * anything else.  One launch on rs_stream() after stream_to_wait (may be NULL); returns after enqueueing. */
int32_t rs_three_view_init_batch_device(rs_ctx* ctx, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const uint32_t* ic,
                                        const uint32_t* i_first, const uint32_t* i_second, const rs_camera* cam,
                                        const void* d_pose_first, const void* d_pose_second, const void* d_triples,
                                        const void* d_ntriples, const void* d_first_only, const void* d_nfirst,
                                        const void* d_second_only, const void* d_nsecond, uint32_t n_scenes,
                                        const rs_three_view_params* params, void* d_pose_out, void* d_verdict, void* d_combined,
                                        void* d_first_ok, void* d_second_ok, void* d_stats, void* stream_to_wait);
/* ---- the three-view constraints of the pose graph on the device ----
 * What cv-sfm's VSlam::optimize_three_view does for ONE covisible view triple of an existing reconstruction
 * (cv-sfm/src/lib.rs:1939-2062), for n_constraints triples side by side: the minimum-landmarks test on the whole list, the
 * relative poses first = pose[v1] * pose[v0]^-1 and second = pose[v2] * pose[v0]^-1, take(optimization_maximum_landmarks),
 * the robust bearing pairs among the taken landmarks, constraint_patience iterations of three_view_adaptive_optimize_l2
 * (cv-optimize/src/three_view_optimizer.rs:203-272; it has no early exit) and the return to the original scale.  One
 * wavefront per constraint, one launch.  The arithmetic is include/akz_three_view_constraint_math.h (compiled for the device
 * and, by the tests, for the host: equal bit for bit); its head lists what is unpinned against the reference — what
 * akz_three_view_math.h lists, the product of two isometries, and the order of the sum over landmarks, which is fixed there.
 * landmarks.shuffle (lib.rs:1968, the caller's RNG) and sort_unstable_by_key (lib.rs:1970, Rust's order among equal
 * observation counts) stay with the caller: a list arrives in the order the reference would walk it in. */
enum {
    RS_TVC_OK = 0,
    RS_TVC_FEW_LANDMARKS = 1,         /* fewer than optimization_minimum_landmarks in the list (lib.rs:1949) */
    RS_TVC_FEW_BEARING_PAIRS = 2,     /* fewer than robust_view_num_robust_bearing_pair (lib.rs:2026) */
    RS_TVC_BAD_INDEX = 3              /* a block >= n_blocks, a feature >= cap_per_img anywhere in the list, or a list range that
                                       * leaves [0, n_lm]: this constraint alone is refused, nothing is read out of bounds */
};
enum {
    RS_TVC_MAX_LANDMARKS = 256,       /* optimization_maximum_landmarks at the most (beyond 64 a wave keeps them in LDS) */
    RS_TVC_MAX_ITERATIONS = 1 << 20,  /* a larger constraint_patience counts as this: the bound that ends every constraint */
    /* d_stats words (u32) of a constraint; a word behind the stage its verdict fell at is 0: */
    RS_TVC_S_LANDMARKS = 0,           /* the length of the list */
    RS_TVC_S_USED = 1,                /* min(length, optimization_maximum_landmarks) */
    RS_TVC_S_PAIRS = 2,               /* robust bearing pairs */
    RS_TVC_S_ORIGINAL_SCALE = 3,      /* [2] |t_first| + |t_second| before the optimiser: the bits of its f64, low word first */
    RS_TVC_S_FINAL_SCALE = 5,         /* [2] the same behind it */
    RS_TVC_S_STAGE = 7,               /* where the verdict fell: 0 indices, 1 minimum landmarks, 2 bearing pairs, 3 the end */
    RS_TVC_STATS = 8
};
typedef struct rs_three_view_constraint_params {
    uint32_t struct_size;                                      /* sizeof(rs_three_view_constraint_params) */
    uint32_t optimization_minimum_landmarks;                   /* 24 */
    uint32_t optimization_maximum_landmarks;                   /* 64; more than RS_TVC_MAX_LANDMARKS: AKZ_E_TOO_LARGE */
    uint32_t constraint_patience;                              /* 4096: the optimiser's iterations, all of which run */
    uint32_t robust_view_num_robust_bearing_pair;              /* 3 */
    double robust_view_bearing_pair_minimum_cosine_distance;   /* 1e-2 */
} rs_three_view_constraint_params;
/* the reference's defaults (cv-sfm/src/settings.rs:332-338, 465-483) */
int32_t rs_three_view_constraint_params_default(rs_three_view_constraint_params* params);
/* Constraint s: views d_views[s] ([n_constraints][3] u32 keypoint blocks of d_kps, [n_blocks][cap_per_img] akz_keypoint as
 * akz_extract_batch_device leaves them; bearing = CameraIntrinsics::calibrate) under the poses d_poses ([n_blocks][12] f64
 * WorldToCamera, as rs_triangulate_landmarks_device reads them); its landmarks are entries d_lm_start[s] .. d_lm_start[s + 1]
 * (d_lm_start [n_constraints + 1] u32, ascending) of d_lm ([n_lm][3] u32, a landmark's feature in each of the three views), in
 * the caller's order.  Every list is a device array: n_constraints is not bound by rs_batch_reserve.
 * Outputs: d_verdict [n_constraints] u32 (RS_TVC_*) and d_stats [n_constraints][RS_TVC_STATS] u32 — always written; d_pose_out
 * [n_constraints][2][12] f64 the two CameraToCamera poses of the constraint — for RS_TVC_OK only, a refused constraint's are
 * left as they were.  The parameters are checked before anything else (a NaN threshold: AKZ_E_INVALID).  One launch on
 * rs_stream() after stream_to_wait (may be NULL); returns after enqueueing. */
int32_t rs_three_view_constraint_batch_device(rs_ctx* ctx, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks,
                                              const void* d_poses, const rs_camera* cam, const void* d_views, const void* d_lm_start,
                                              const void* d_lm, uint32_t n_lm, uint32_t n_constraints,
                                              const rs_three_view_constraint_params* params, void* d_pose_out, void* d_verdict,
                                              void* d_stats, void* stream_to_wait);
/* ---- the relaxation of the pose graph under its three-view constraints on the device ----
 * What cv-sfm's VSlam::apply_constraints does (cv-sfm/src/lib.rs:2358-2375) for n_graphs reconstructions side by side:
 * optimization_iterations rounds, in each of which every view moves by graph_optimization_rate times the sum, over the edges
 * of its row, of se3(expected_other_to_view * world_to_other * world_to_view^-1) (constrain_view, lib.rs:1892-1936).  A round
 * is a Jacobi sweep: every view reads the poses of the round before.  The chain constraints -> edges -> relaxed WorldToCamera
 * table -> landmark table runs on rs_stream() without a host step: rs_three_view_constraint_batch_device,
 * rs_pose_graph_edges_device, rs_pose_graph_relax_batch_device, rs_triangulate_landmarks_device.
 * The arithmetic is include/akz_pose_graph_math.h (compiled for the device and, by the tests, for the host: equal bit for
 * bit); its head lists what is unpinned against the reference — the log map, the f64 acos, the order of a view's edges and
 * the order of the sum over them, which is fixed there: one wavefront per view, whichever kernel runs the graph.
 * A small graph is relaxed by one persistent workgroup with both pose tables in LDS (k_pg_relax_resident; it can hold
 * RS_PG_RESIDENT_VIEWS views and takes graphs of at most RS_PG_DEFAULT_RESIDENT_VIEWS, where it is the faster form), a
 * larger one by one launch per round over its views (k_pg_relax_sweep), the tables ping-ponging between d_poses and scratch
 * of the context; the two give equal bits.  The graphs of one call may not overlap.
 * The reference indexes a removed view in the round after it removed one for a non-finite delta and panics (slotmap): a
 * graph stops here at the first round with such a view and says so (RS_PG_NONFINITE). */
enum {
    RS_PG_OK = 0,
    RS_PG_FEW_VIEWS = 1,              /* fewer than 3 views would be updated (lib.rs:2413): decided before round 0, poses untouched */
    RS_PG_NONFINITE = 2,              /* round k = RS_PG_S_ROUNDS - 1 was the first in which a view's net delta was not finite
                                       * (lib.rs:1929): the finite views' updates of that round are installed, the view is
                                       * RS_PG_VIEW_NONFINITE, the graph stopped.  k + 1 == iterations: the reference would have
                                       * returned with that view removed; anything earlier: the reference panics */
    RS_PG_BAD_INDEX = 3               /* a row entry >= 6 * n_constraints; an entry of an accepted constraint whose target is not
                                       * the row's view or whose other view lies outside the graph's range; a start array that is
                                       * not ascending within [0, n_rows] / [0, n_views]: this graph alone is refused, its poses
                                       * and view states untouched, nothing is read out of bounds.  For d_graph_start "not
                                       * ascending" reaches back: a graph is refused as well when any start in front of it lies
                                       * above its own ([0, 6, 4, 10]: [6, 4) and [4, 10) are refused, [0, 6) is not), so the
                                       * graphs that run never share a view */
};
enum {
    RS_PG_VIEW_UPDATED = 0,
    RS_PG_VIEW_NO_CONSTRAINT = 1,     /* no edge of an RS_TVC_OK constraint in the view's row (lib.rs:1900-1902): pose untouched */
    RS_PG_VIEW_NONFINITE = 2
};
enum {
    RS_PG_RESIDENT_VIEWS = 256,       /* the most the resident form can take: two pose tables of so many views are 48 KB of the
                                       * 64 KB of static LDS */
    RS_PG_DEFAULT_RESIDENT_VIEWS = 8, /* the most it takes unless told otherwise: one wave per view.  Measured: a
                                       * view's round is a 5 us chain of FP64 latency, the 8 waves of the workgroup walk a graph's
                                       * views in turns, a launch per round costs 7 us for any number of views.  A limit this
                                       * small holds for the CALL: with more than 8 views in it the launches per round are
                                       * enqueued anyway and take every graph, so by default the resident form serves calls of at
                                       * most 8 views in all and nothing else */
    RS_PG_MAX_ITERATIONS = 1 << 20,   /* a larger optimization_iterations counts as this */
    /* d_stats words (u32) of a graph; a word behind the stage its verdict fell at is 0: */
    RS_PG_S_VIEWS = 0,                /* the views the graph owns */
    RS_PG_S_UPDATED = 1,              /* those with an edge of an accepted constraint in their row */
    RS_PG_S_EDGES = 2,                /* row entries of accepted constraints over all its rows */
    RS_PG_S_ROUNDS = 3,               /* rounds run */
    RS_PG_S_STAGE = 4,                /* where the verdict fell: 0 indices, 1 the count of views, 2 the rounds */
    RS_PG_S_FIRST_BAD_VIEW = 5,       /* the lowest view whose net was not finite, 0xFFFFFFFF when there is none */
    RS_PG_STATS = 8                   /* words 6 and 7 are 0 */
};
typedef struct rs_pose_graph_params {
    uint32_t struct_size;                                      /* sizeof(rs_pose_graph_params) */
    uint32_t optimization_iterations;                          /* 1024 */
    double graph_optimization_rate;                            /* 1e-3; NaN or infinite: AKZ_E_INVALID */
} rs_pose_graph_params;
/* the reference's defaults (cv-sfm/src/settings.rs:461-463, 477-479) */
int32_t rs_pose_graph_params_default(rs_pose_graph_params* params);
/* ThreeViewConstraint::edge_constraints (lib.rs:167-180) for every constraint of an rs_three_view_constraint_batch_device
 * call: from its d_views, d_pose_out (d_constraint_poses) and d_verdict, d_edges [n_constraints][6][12] f64, the expected
 * other-to-target isometries in the slot order {second^-1, first^-1, first, (second first^-1)^-1, second first^-1, second}.
 * Slot s has target view d_views[c][T[s]] and other view d_views[c][O[s]], T = {0,0,1,1,2,2}, O = {2,1,0,2,1,0}.  A
 * constraint whose verdict is not RS_TVC_OK gets six zero matrices (its poses are not read).  One launch on rs_stream(). */
int32_t rs_pose_graph_edges_device(rs_ctx* ctx, const void* d_views, const void* d_constraint_poses, const void* d_constraint_verdict,
                                   uint32_t n_constraints, void* d_edges, void* stream_to_wait);
/* d_poses [n_views][12] f64: the WorldToCamera table rs_triangulate_landmarks_device reads, updated in place.  Graph g owns
 * views d_graph_start[g] .. d_graph_start[g + 1] (u32 [n_graphs + 1]); view v's row is entries d_row_start[v] ..
 * d_row_start[v + 1] (u32 [n_views + 1]) of d_row_edges (u32 [n_rows]), each an edge id 6 * constraint + slot, in the
 * caller's order (the reference walks a HashMap and defines none).  d_views, d_constraint_verdict and d_edges are those of
 * rs_pose_graph_edges_device.  Every list is a device array: n_views and n_constraints are not bound by rs_batch_reserve.
 * Outputs: d_graph_verdict [n_graphs] u32 (RS_PG_*) and d_stats [n_graphs][RS_PG_STATS] u32 — always written; d_view_state
 * [n_views] u32 (RS_PG_VIEW_*) — the views of every graph but a RS_PG_BAD_INDEX one.  The parameters are checked before
 * anything else.  Enqueues on rs_stream() after stream_to_wait (may be NULL) and returns; no host synchronisation between
 * rounds. */
int32_t rs_pose_graph_relax_batch_device(rs_ctx* ctx, void* d_poses, uint32_t n_views, const void* d_graph_start, uint32_t n_graphs,
                                         const void* d_row_start, const void* d_row_edges, uint32_t n_rows, const void* d_views,
                                         const void* d_constraint_verdict, const void* d_edges, uint32_t n_constraints,
                                         const rs_pose_graph_params* params, void* d_graph_verdict, void* d_view_state, void* d_stats,
                                         void* stream_to_wait);
/* parity tap: graphs of more than `views` views (at most RS_PG_RESIDENT_VIEWS; RS_PG_DEFAULT_RESIDENT_VIEWS when never
 * called) take the swept form in the calls that follow on this context — 0 sends every graph through it; with a limit of
 * at most 8 a call of more views than the limit is swept as a whole */
int32_t rs_pose_graph_debug_resident_views(rs_ctx* ctx, uint32_t views);
/* ---- the observation filter behind a relaxation, and optimize_reconstruction as a whole, on the device ----
 * What cv-sfm's VSlam::filter_non_robust_observations does (cv-sfm/src/lib.rs:2657-2757) for n_recons reconstructions side by
 * side: every landmark is triangulated again under the poses as they are now, the observations that no longer agree with
 * their landmark are split off, landmarks that no longer triangulate are split whole, and a reconstruction that keeps fewer
 * than minimum_robust_landmarks robust landmarks is rejected.  One lane per landmark decides (the design matrix and the
 * eigenvectors in registers, one keep flag per observation in memory); an exclusive scan of the keep flags over the
 * observations of the call — tile sums, a scan of the tile sums by one workgroup, a scatter; no workgroup waits for another —
 * builds the filtered table and the list of the split-off observations.  The arithmetic is
 * include/akz_observation_filter_math.h (compiled for the device and, by the tests, for the host: equal bit for bit); its
 * head lists what is unpinned against the reference — above all the order of a landmark's observations, which decides which
 * observation a split leaves behind. */
enum {                                /* d_lm_state: what became of a landmark */
    RS_OF_KEPT = 0,                   /* two or more observations, all stayed */
    RS_OF_SINGLE = 1,                 /* one observation or none: nothing happens (lib.rs:2686-2687) */
    RS_OF_PAIR_SPLIT = 2,             /* two observations that failed is_bi_landmark_robust: the second was split off */
    RS_OF_NO_POINT = 3,               /* three or more and no point (d_tri_reason says why): all but the first were split off */
    RS_OF_KICKED = 4,                 /* three or more, a point, at least one observation split off */
    RS_OF_BAD_INDEX = 5,              /* an observation names a block >= n_blocks or a feature >= cap_per_img: the landmark is left
                                       * as it is and is not robust, nothing is read out of bounds */
    RS_OF_SKIPPED = 6                 /* the landmark belongs to no reconstruction that ran (d_skip, a refused range, or no range
                                       * at all): left as it is, nothing computed */
};
enum {                                /* d_recon_verdict */
    RS_OF_OK = 0,
    RS_OF_FEW_LANDMARKS = 1,          /* fewer than minimum_robust_landmarks robust after the filter (lib.rs:2747-2753): the reference
                                       * removes the reconstruction; here its filtered table is still written */
    RS_OF_BAD_RANGE = 2,              /* d_recon_start, d_view_start or the part of d_obs_start the reconstruction owns is not
                                       * ascending inside its bounds ([0, n_landmarks], [0, n_blocks], [0, n_obs]), or a start in
                                       * front of the range lies above its first (as RS_PG_BAD_INDEX reaches back): this
                                       * reconstruction alone is refused and passes through, so the ones that run never share an
                                       * observation */
    RS_OF_RECON_SKIPPED = 3           /* d_skip[r] != 0: passed through */
};
enum {
    RS_OF_NO_SOLVE = 255,             /* d_tri_reason of a landmark whose filter ran no triangulation */
    RS_OF_ROBUST_BEFORE = 1,          /* d_robust bit 0: is_landmark_robust before the filter */
    RS_OF_ROBUST_AFTER = 2,           /* d_robust bit 1: after it */
    /* d_stats words (u32) of a reconstruction; all 0 for RS_OF_BAD_RANGE, all but the first 0 for RS_OF_RECON_SKIPPED: */
    RS_OF_S_LANDMARKS = 0,            /* rows of the table it owns */
    RS_OF_S_ROBUST_BEFORE = 1,        /* initial_num_landmarks (lib.rs:2670-2676) */
    RS_OF_S_ROBUST_AFTER = 2,         /* final_num_landmarks (lib.rs:2738-2744) */
    RS_OF_S_OBS_SPLIT = 3,            /* observations split off */
    RS_OF_S_PAIR_SPLIT = 4,           /* landmarks RS_OF_PAIR_SPLIT */
    RS_OF_S_NO_POINT = 5,             /* landmarks RS_OF_NO_POINT */
    RS_OF_S_KICKED = 6,               /* landmarks RS_OF_KICKED */
    RS_OF_STATS = 8,                  /* word 7 is 0 */
    RS_OF_MAX_ITERATIONS = 64,        /* a larger reconstruction_optimization_iterations: AKZ_E_TOO_LARGE */
    /* d_verdict of rs_optimize_reconstruction_batch_device: 0, or RS_OR_STOPPED | round << 16 | stage << 8 | the verdict the
     * stage gave (RS_PG_* or RS_OF_*) */
    RS_OR_OK = 0,
    RS_OR_STAGE_RELAX = 1,
    RS_OR_STAGE_FILTER = 2,
    RS_OR_STOPPED = 1 << 30
};
typedef struct rs_observation_filter_params {
    uint32_t struct_size;                                /* sizeof(rs_observation_filter_params) */
    uint32_t minimum_robust_landmarks;                   /* 32 */
    double maximum_cosine_distance;                      /* 1e-5; NaN: AKZ_E_INVALID */
    double maximum_sine_distance;                        /* 1e-1; NaN: AKZ_E_INVALID */
    uint32_t reconstruction_optimization_iterations;     /* 1: the rounds of rs_optimize_reconstruction_batch_device */
    uint32_t reserved;                                   /* 0 */
    rs_triangulate_params triangulate;                   /* the eigen-solver's settings, robust_minimum_observations and the incidence
                                                          * distance; its n_views is used by the closing triangulation of
                                                          * rs_optimize_reconstruction_batch_device only: the filter takes every
                                                          * reconstruction's own from d_view_start */
} rs_observation_filter_params;
/* the reference's defaults (cv-sfm/src/settings.rs:324-350, 429-431) */
int32_t rs_observation_filter_params_default(rs_observation_filter_params* params);
/* One pass of the filter.  The landmark table as rs_triangulate_landmarks_device takes it (d_kps, cap_per_img, n_blocks,
 * d_poses, cam, d_obs_start [n_landmarks + 1], d_obs [n_obs][2]; a block is a view); only the first min(d_obs_start[n_landmarks],
 * n_obs) observations are the table's, so n_obs may be the capacity of an array whose fill is known on the device only.
 * Reconstruction r owns landmarks d_recon_start[r] .. d_recon_start[r + 1] (u32 [n_recons + 1]) and has d_view_start[r + 1] -
 * d_view_start[r] views (u32 [n_recons + 1], the d_graph_start of rs_pose_graph_relax_batch_device).  d_skip (optional)
 * [n_recons] u32: nonzero = pass the reconstruction through.
 * Outputs, all written by every call: d_keep [n_obs] u8 (1 = the observation stays; everything outside a running
 * reconstruction is 1), d_lm_state [n_landmarks] u8 (RS_OF_*), d_tri_reason [n_landmarks] u8 (RS_TRI_* of
 * triangulate_landmark where it ran, 6 for a bad index, RS_OF_NO_SOLVE otherwise), d_robust [n_landmarks] u8 (bits
 * RS_OF_ROBUST_*), d_recon_verdict [n_recons] u32, d_stats [n_recons][RS_OF_STATS] u32, d_counts [2] u32 {observations kept,
 * observations split off}, and the two compacted lists: the filtered table d_obs_start_out [n_landmarks + 1] / d_obs_out
 * (room for [n_obs][2]; rows [0, kept) are written: the kept observations of every landmark in their order) and d_split_out
 * (room for [n_obs][2]; rows [0, split) are written: the split-off observations in (landmark, position) order — the k-th of
 * them is by definition the new single-observation landmark n_landmarks + k).  The input table is const: an output that
 * overlaps d_obs_start or d_obs is refused with AKZ_E_INVALID before anything is enqueued.  The parameters are checked before
 * anything else.  Enqueues on rs_stream() after stream_to_wait (may be NULL) and returns; allocates nothing beyond growing the
 * context's scratch. */
int32_t rs_filter_observations_device(rs_ctx* ctx, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses,
                                      const rs_camera* cam, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
                                      uint32_t n_landmarks, const void* d_recon_start, const void* d_view_start, uint32_t n_recons,
                                      const void* d_skip, const rs_observation_filter_params* params, void* d_keep, void* d_lm_state,
                                      void* d_tri_reason, void* d_robust, void* d_obs_start_out, void* d_obs_out, void* d_split_out,
                                      void* d_counts, void* d_recon_verdict, void* d_stats, void* stream_to_wait);
/* VSlam::optimize_reconstruction (cv-sfm/src/lib.rs:2343-2355) for n_graphs reconstructions side by side:
 * reconstruction_optimization_iterations rounds of rs_pose_graph_relax_batch_device (its arguments, d_poses ... pg_params, with
 * n_views == the n_blocks of the landmark table and d_graph_start as the filter's d_view_start) followed by
 * rs_filter_observations_device on the table the round before wrote, without a host step between them.  A reconstruction
 * whose graph verdict is not RS_PG_OK, or which the filter rejects, stops there: d_verdict [n_graphs] u32 says which round
 * and which stage (RS_OR_*), its poses are not relaxed again and the filters of later rounds pass its part of the table
 * through.  (The reference removes such a reconstruction; and it lets a graph whose view was removed in the LAST round of a
 * relaxation through to the filter — DESIGN.md §7 —, which this call does not follow: RS_PG_NONFINITE stops a reconstruction
 * in whichever round it falls.)
 * Outputs: d_graph_verdict, d_view_state, d_pg_stats as the relaxation writes them, of the last round a reconstruction was
 * relaxed in; d_recon_verdict [iterations][n_graphs] and d_of_stats [iterations][n_graphs][RS_OF_STATS] of every round's
 * filter; d_split_out [iterations][n_obs][2] and d_counts [iterations][2] likewise (round k's split-off observations are
 * the single-observation landmarks the later rounds do not see: they can never become robust again); d_keep, d_lm_state,
 * d_tri_reason, d_robust of the LAST round, d_keep indexing the table that round read; d_obs_start_out / d_obs_out the final
 * table.  The tables between the rounds live in scratch of the context (two of them at the most, grown on demand); with one
 * iteration there is none.  d_world (optional) [n_landmarks][4] f64 and d_world_reason (optional) [n_landmarks] u8:
 * rs_triangulate_landmarks_device on the final table, so that the world table the registration chain reads is the filtered
 * one.  iterations == 0 copies the table to the outputs and triangulates it. */
int32_t rs_optimize_reconstruction_batch_device(rs_ctx* ctx, void* d_poses, uint32_t n_views, const void* d_graph_start, uint32_t n_graphs,
                                                const void* d_row_start, const void* d_row_edges, uint32_t n_rows, const void* d_views,
                                                const void* d_constraint_verdict, const void* d_edges, uint32_t n_constraints,
                                                const rs_pose_graph_params* pg_params, const void* d_kps, uint32_t cap_per_img,
                                                const rs_camera* cam, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
                                                uint32_t n_landmarks, const void* d_recon_start,
                                                const rs_observation_filter_params* params, void* d_verdict, void* d_graph_verdict,
                                                void* d_view_state, void* d_pg_stats, void* d_keep, void* d_lm_state, void* d_tri_reason,
                                                void* d_robust, void* d_obs_start_out, void* d_obs_out, void* d_split_out, void* d_counts,
                                                void* d_recon_verdict, void* d_of_stats, void* d_world, void* d_world_reason,
                                                void* stream_to_wait);
/* ---- the covisibility search in front of the three-view constraints, their record and the rows of the pose graph ----
 * What cv-sfm's VSlam::generate_view_constraints does up to its call of optimize_three_view (cv-sfm/src/lib.rs:2438-2516, with
 * view_covisibilities, lib.rs:2535-2556), the verdict of record_view_constraints (lib.rs:2092-2109) and flatten_constraints
 * (lib.rs:2519-2532), so that landmark table -> candidates -> constraints -> recorded set -> edges -> rows ->
 * rs_optimize_reconstruction_batch_device runs on rs_stream() without a host step (regenerate_reconstruction, lib.rs:2418-2435).
 * Integers only.  The decisions are include/akz_covisibility_math.h (compiled for the device and, by the tests, for the host:
 * equal in every word); its head lists the admissible order it fixes where the reference walks HashMaps and sorts unstably. */
enum {                                /* d_target_verdict */
    RS_CV_OK = 0,
    RS_CV_FEW_CONSTRAINTS = 1,        /* record: fewer than optimization_minimum_new_constraints recorded and recorded + 1 < the
                                       * views of the target's reconstruction (lib.rs:2098-2102): nothing of the target is recorded */
    RS_CV_BAD_INDEX = 2,              /* the target is >= n_blocks; a landmark of one of its features names a block >= n_blocks or a
                                       * feature >= cap_per_img; or some start pair of d_obs_start does not ascend within [0, n_obs]
                                       * (which refuses every target of the call): no slot is filled, nothing is read out of bounds */
    RS_CV_NO_GRAPH = 3                /* record: no range of d_graph_start holds the target */
};
enum {
    RS_CV_NOT_RECORDED = 16,          /* d_recorded of a slot the constraint stage accepted and the record did not take */
    RS_CV_MAX_CANDIDATE_VIEWS = 128,  /* candidate views of a target: 8 128 pairs, whose sort keys are 64 KB of LDS, and 128 bit rows
                                       * of scratch per workgroup; a target with more keeps the largest counts, ties to the lower
                                       * block, and says so (RS_CV_F_CANDIDATES_CAPPED) */
    RS_CV_MAX_SLOTS = 256,            /* candidate_limit at the most: a target's slots are walked by one lane */
    RS_CV_MAX_FEATURES = 8192,        /* cap_per_img at the most: AKZ_E_TOO_LARGE beyond (a list's sort keys live in LDS) */
    /* d_stats words (u32) of a target; all 0 for RS_CV_BAD_INDEX: */
    RS_CV_S_ROBUST = 0,               /* features whose landmark is robust */
    RS_CV_S_CANDIDATES = 1,           /* candidate views kept */
    RS_CV_S_PAIRS = 2,                /* triples at or above optimization_robust_covisibility_minimum_landmarks */
    RS_CV_S_UNIQUE = 3,               /* triples the unique walk took (lib.rs:2490-2495) */
    RS_CV_S_EMITTED = 4,              /* slots filled */
    RS_CV_S_FLAGS = 5,                /* RS_CV_F_* */
    RS_CV_S_RECORDED = 6,             /* constraints recorded: 0 from the candidates call, written by the record */
    RS_CV_STATS = 8,                  /* word 7 is 0 */
    RS_CV_F_CANDIDATES_CAPPED = 1,
    RS_CV_F_LIMIT_REACHED = 2         /* the chain held further admissible triples beyond the limit: the reference would try them
                                       * after a refusal by the constraint stage; run again with a larger candidate_limit */
};
typedef struct rs_covisibility_params {
    uint32_t struct_size;                                             /* sizeof(rs_covisibility_params) */
    uint32_t optimization_robust_covisibility_minimum_landmarks;      /* 16 */
    uint32_t optimization_maximum_three_view_constraints;             /* 64 */
    uint32_t optimization_minimum_new_constraints;                    /* 4 */
    uint32_t optimization_minimum_landmarks;                          /* 24; above the maximum: AKZ_E_INVALID */
    uint32_t optimization_maximum_landmarks;                          /* 64; more than RS_TVC_MAX_LANDMARKS: AKZ_E_TOO_LARGE */
    uint32_t candidate_limit;                                         /* 0: slots per target; 0 = the maximum of constraints; more
                                                                       * than RS_CV_MAX_SLOTS either way: AKZ_E_TOO_LARGE */
    uint32_t shuffle_seed;                                            /* 0: ties of a list's sort by position; else by a mix of
                                                                       * (seed, landmark), in place of lib.rs:1968's shuffle */
} rs_covisibility_params;
/* the reference's defaults (cv-sfm/src/settings.rs:453-475) */
int32_t rs_covisibility_params_default(rs_covisibility_params* params);
/* The landmark table as rs_triangulate_landmarks_device takes it (d_obs_start [n_landmarks + 1], d_obs [n_obs][2], cap_per_img,
 * n_blocks) and d_reason [n_landmarks] u8 as that call writes it: a landmark is robust iff its byte is RS_TRI_OK.  d_targets
 * [n_targets] u32: the views (keypoint blocks) to generate constraints for.  With limit = candidate_limit, or
 * optimization_maximum_three_view_constraints when that is 0, target t owns slots t * limit .. (t + 1) * limit of
 * d_views [n_slots][3], d_lm_start [n_slots + 1] and d_lm [n_slots * optimization_maximum_landmarks][3], the arrays
 * rs_three_view_constraint_batch_device reads (n_constraints = n_slots, n_lm = n_slots * optimization_maximum_landmarks).  All
 * outputs are written in full (d_lm behind the last list with zeros).  An unused slot has views {0, 0, 0} and an empty list, which
 * the constraint stage refuses with RS_TVC_FEW_LANDMARKS.  d_slot_count [n_slots] u32: a slot's covisible landmarks before the
 * cut to optimization_maximum_landmarks; d_target_verdict [n_targets] u32 (RS_CV_OK or RS_CV_BAD_INDEX); d_stats
 * [n_targets][RS_CV_STATS] u32.  The parameters are checked before anything else.  Enqueues on rs_stream() after stream_to_wait
 * (may be NULL) and returns; allocates nothing beyond growing the context's scratch. */
int32_t rs_covisibility_candidates_device(rs_ctx* ctx, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks,
                                          uint32_t cap_per_img, uint32_t n_blocks, const void* d_reason, const void* d_targets,
                                          uint32_t n_targets, const rs_covisibility_params* params, void* d_views, void* d_lm_start,
                                          void* d_lm, void* d_slot_count, void* d_target_verdict, void* d_stats, void* stream_to_wait);
/* Behind rs_three_view_constraint_batch_device on those slots: d_constraint_verdict [n_slots] u32 is its d_verdict.  Per target,
 * in slot order, the first optimization_maximum_three_view_constraints RS_TVC_OK slots are recorded (lib.rs:2511-2514) unless
 * record_view_constraints' rule refuses the target; the views of its reconstruction are the length of the first range of
 * d_graph_start [n_graphs + 1] (rs_pose_graph_relax_batch_device's) that holds it.  d_recorded [n_slots] u32: RS_TVC_OK for a
 * recorded constraint, else the constraint's own verdict or RS_CV_NOT_RECORDED — what rs_pose_graph_edges_device and the
 * relaxation take as d_constraint_verdict.  d_target_verdict and d_stats are the candidates call's, updated in place: a target
 * that is RS_CV_BAD_INDEX stays so and records nothing, the others become RS_CV_OK, RS_CV_FEW_CONSTRAINTS or RS_CV_NO_GRAPH;
 * word RS_CV_S_RECORDED is written. */
int32_t rs_covisibility_record_device(rs_ctx* ctx, const void* d_constraint_verdict, const void* d_targets, uint32_t n_targets,
                                      const void* d_graph_start, uint32_t n_graphs, const rs_covisibility_params* params, void* d_recorded,
                                      void* d_target_verdict, void* d_stats, void* stream_to_wait);
/* flatten_constraints: d_row_start [n_views + 1] and d_row_edges [6 * n_constraints] u32 of rs_pose_graph_relax_batch_device from
 * d_views [n_constraints][3]: view v's row holds the edge ids 6 * constraint + slot whose target is v in ascending order.
 * Refused constraints stay in the rows.  A triple that names a view >= n_views contributes nothing and sets d_flags [1] u32 to 1
 * (0 otherwise); d_row_edges behind d_row_start[n_views] is 0.  The triples behind rs_repack_constraints_device's count (views
 * 0xFFFFFFFF) are skipped this way: with that call's room as n_constraints the rows are those of the count, and the flag reads 1. */
int32_t rs_pose_graph_rows_device(rs_ctx* ctx, const void* d_views, uint32_t n_constraints, uint32_t n_views, void* d_row_start,
                                  void* d_row_edges, void* d_flags, void* stream_to_wait);
/* ---- the refinement of registered poses on the device: single-view L2 optimiser and consistency filter ----
 * What cv-sfm's register_frame_subset does behind its consensus (cv-sfm/src/lib.rs:1625-1775), for the new frames of a
 * micro-batch side by side — the same scenes as the preceding rs_p3p_arrsac_batch_device call: the first
 * single_view_optimization_num_matches inliers, single_view_simple_optimize_l2 (cv-optimize/src/single_view_optimizer.rs:
 * 80-135), the re-selection of the original matches that are is_observation_consistent (lib.rs:2622-2655) under the new pose
 * and have a robust world point, single_view_filter_loop_iterations times, one more optimisation, and the final counts and
 * the map of consistent matches.  One persistent workgroup per scene, one launch.  The arithmetic is
 * include/akz_single_view_math.h (compiled for the device and, by the tests, for the host: equal bit for bit); its head lists
 * what is unpinned against the reference — the order of the sum over matches, which is fixed there, among it. */
enum {
    RS_SV_OK = 0,
    RS_SV_NO_MODEL = 1,        /* the consensus found no pose (d_best_id == 0xFFFFFFFF): passed through, the pose copied */
    RS_SV_FEW_LANDMARKS = 2,   /* fewer than single_view_minimum_landmarks matches with a world point (lib.rs:1606) */
    RS_SV_LOST_HALF = 3,       /* no more than half of the inliers taken are left (lib.rs:1650, 1697, 1737) */
    RS_SV_FEW_ROBUST = 4,      /* fewer than single_view_minimum_robust_landmarks final matches (lib.rs:1766) */
    RS_SV_BAD_INDEX = 5        /* a match, a landmark, an observation or an inlier names something outside the caller's arrays:
                                * the scene is refused, nothing is read out of bounds */
};
enum {
    RS_SV_MAX_MATCHES = 2048,         /* single_view_optimization_num_matches at the most (they live in one workgroup's LDS) */
    RS_SV_MAX_RUNS = 9,               /* single_view_filter_loop_iterations + 1 at the most */
    RS_SV_MAX_ITERATIONS = 1 << 20,   /* a larger single_view_patience counts as this: the bound that ends every run */
    /* d_stats words (u32) of a scene: */
    RS_SV_S_INLIERS = 0,              /* inliers taken */
    RS_SV_S_RUN_MATCHES = 1,          /* [9] matches entering run r; 0xFFFFFFFF: not reached */
    RS_SV_S_RUN_STOP = 10,            /* [9] the iteration run r left its loop at (patience - 1: the last one; less: 50 iterations
                                       * without improvement); 0xFFFFFFFF: not run */
    RS_SV_S_ROBUST = 19,              /* final_num_robust_matches */
    RS_SV_S_NO_OTHER = 20,            /* original matches whose landmarks have no observation ("unreachable" in the reference; never
                                       * consistent here) */
    RS_SV_S_STAGE = 21,               /* where the verdict fell: 0 indices, 1 minimum landmarks, 2 the model, 3 + r entering run r,
                                       * 12 final_num_robust_matches, 13 the final matches (and RS_SV_OK) */
    RS_SV_STATS = 24
};
typedef struct rs_single_view_params {
    uint32_t struct_size;                              /* sizeof(rs_single_view_params) */
    uint32_t single_view_optimization_num_matches;     /* 2048; more than RS_SV_MAX_MATCHES: AKZ_E_TOO_LARGE */
    uint32_t single_view_filter_loop_iterations;       /* 5; more than RS_SV_MAX_RUNS - 1: AKZ_E_TOO_LARGE */
    uint32_t single_view_patience;                     /* 100000: the optimiser's iteration limit */
    double single_view_optimization_rate;              /* 1e-3 */
    uint32_t single_view_minimum_landmarks;            /* 32 */
    uint32_t single_view_minimum_robust_landmarks;     /* 64 */
    double maximum_cosine_distance;                    /* 1e-5 */
    double maximum_sine_distance;                      /* 1e-1 */
    rs_triangulate_params triangulate;                 /* the eigen-solver's settings (max_sweeps, eps) */
} rs_single_view_params;
/* the reference's defaults (cv-sfm/src/settings.rs:324-383) */
int32_t rs_single_view_params_default(rs_single_view_params* params);
/* Scene s < n_scenes is the new frame in keypoint block ik[s] of d_kps.  The landmark table as rs_triangulate_landmarks_device
 * takes it (d_kps, cap_per_img, n_blocks, d_poses of the views, cam, d_obs_start [n_landmarks + 1], d_obs [n_obs][2]) and the
 * world table d_world / n_world the consensus read (with n_world + n_scenes * cap_per_img rows when d_best is given).
 * d_matches [n_scenes][cap_per_img][2] u32 {feature, world row} with d_nmatches [n_scenes]: the ORIGINAL matches in their order
 * (lib.rs:1549-1576; hm_landmark_original_matches_batch_device), those whose world row says "None" (w < 0) included.  A row
 * < n_world is the landmark of that key; a row n_world + f * cap_per_img + j is the merged match of d_best[f][j][0..1] (d_best
 * as hm_best_of_views_batch_device leaves it; optional, required only when such a row occurs), whose observations are those
 * of its first landmark followed by those of its second.  d_pose, d_best_id, d_inliers, d_n_inliers: the consensus' outputs;
 * inlier index k names the k-th entry of d_matches whose world row has w >= 0, in order — the list
 * hm_landmark_matches_*_batch_device hands the consensus for the same world table.
 * Outputs per scene: d_pose_out [12] f64 (written for RS_SV_OK and, as a copy, RS_SV_NO_MODEL), d_verdict u32 (RS_SV_*),
 * d_final [cap_per_img] u8 (1 where original match i is consistent under the final pose: the final_matches map; written for
 * the matches of the scene once the final pass is reached), d_n_final u32 (0 before that), d_stats [RS_SV_STATS] u32.
 * A scene that names a feature, world row, landmark, block or observation range outside the caller's arrays, or an inlier
 * beyond its robust sub-list, is refused alone (RS_SV_BAD_INDEX).  The parameters are checked before anything else (a NaN
 * threshold: AKZ_E_INVALID).  n_scenes within rs_batch_reserve's room.  One launch on rs_stream() after stream_to_wait (may
 * be NULL); returns after enqueueing; allocates nothing beyond growing the context's scratch. */
int32_t rs_refine_poses_batch_device(rs_ctx* ctx, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses,
                                     const rs_camera* cam, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
                                     uint32_t n_landmarks, const void* d_world, uint32_t n_world, const uint32_t* ik,
                                     const void* d_matches, const void* d_nmatches, const void* d_best, const void* d_pose,
                                     const void* d_best_id, const void* d_inliers, const void* d_n_inliers, uint32_t n_scenes,
                                     const rs_single_view_params* params, void* d_pose_out, void* d_verdict, void* d_final,
                                     void* d_n_final, void* d_stats, void* stream_to_wait);
/* ---- the landmark table of a reconstruction on the device: the graph test behind a merge, add_view for a micro-batch ----
 * What cv-sfm keeps on the host between the registration of a frame and the next generation of its landmarks
 * (VSlam::are_landmarks_sharing_view, cv-sfm/src/lib.rs:1435-1449; VSlamData::add_view, add_landmark and merge_landmarks,
 * lib.rs:432-500, 699-721).  Integer data movement over the table rs_triangulate_landmarks_device reads; the decisions are
 * include/akz_landmark_table_math.h (compiled for the device and, by the tests, for the host: equal byte for byte), whose head
 * lists the departures from the reference — the rule for two frames of one call that name one landmark among them. */
enum {
    RS_AV_OK = 0,
    RS_AV_NOT_ACCEPTED = 1,    /* the slot's refinement verdict is not RS_SV_OK, d_skip names it, or the call was refused */
    RS_AV_BAD_INDEX = 2,       /* a count above cap_per_img, a final match that names nothing, or a feature in two final matches:
                                * the slot is refused alone and contributes nothing */
    RS_AV_BAD_TABLE = 3,       /* d_call_verdict only: the starts of the input table do not ascend inside [0, n_obs] */
    /* d_stats words (u32) of a slot: */
    RS_AV_S_OBSERVATIONS = 0,  /* observations added to rows of the input table (its final matches) */
    RS_AV_S_MERGED = 1,        /* merges applied */
    RS_AV_S_DEMOTED = 2,       /* merges demoted: the observation went to the first landmark alone */
    RS_AV_S_NEW_LANDMARKS = 3, /* rows added behind the table (its features in no final match) */
    RS_AV_STATS = 4,
    RS_AV_COUNTS = 4,          /* d_counts_out: {rows filled, observations filled, merges applied, merges demoted} */
    RS_LT_TILE = 1024          /* rows of the input table one workgroup scans (the tests walk its boundaries) */
};
/* are_landmarks_sharing_view for every merge candidate of a micro-batch.  The landmark table as
 * rs_triangulate_landmarks_device takes it (d_obs_start [n_landmarks + 1], d_obs [n_obs][2] {block, feature}; the table fills
 * the first min(d_obs_start[n_landmarks], n_obs) observations); d_best [n_frames][cap_per_img][3]{landmark, distance} and
 * d_decision [n_frames][cap_per_img] as hm_best_of_views_batch_device leaves them.  d_merge_ok [n_frames][cap_per_img] u8, every
 * byte written: 1 iff the decision is 2, best[0] and best[1] are below n_landmarks, both lists lie inside the table and share no
 * block; 0 otherwise (an absent landmark, 0xFFFFFFFF, included).  Nothing is read out of bounds.  The mask is what
 * rs_triangulate_merged_device and hm_landmark_matches_*_batch_device take.  n_frames <= 65535.  One launch on rs_stream() after
 * stream_to_wait (may be NULL); returns after enqueueing. */
int32_t rs_landmarks_sharing_view_device(rs_ctx* ctx, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks,
                                         const void* d_best, const void* d_decision, uint32_t cap_per_img, uint32_t n_frames,
                                         void* d_merge_ok, void* stream_to_wait);
/* add_view for the accepted frames of a micro-batch and the rows of the observation filter's split list: the next generation of
 * the table, out of place (an output array that overlaps d_obs_start or d_obs: AKZ_E_INVALID).
 * Inputs: the table (d_obs_start, d_obs, n_obs, n_landmarks); n_world, the row numbering of d_matches (as in
 * rs_refine_poses_batch_device; a row below n_world but not below n_landmarks names nothing); the optional split list d_split
 * [split_room][2] with its length d_split_count [1] u32 on the device (rs_filter_observations_device's d_split_out and
 * d_counts[1]; both NULL and split_room 0 for none).  Slot f < n_frames is the frame in keypoint block ik[f] (a host list of
 * distinct blocks below n_blocks, else AKZ_E_INVALID) with what the refinement left on the device: d_counts [n_blocks] u32 the
 * feature counts, d_matches [n_frames][cap_per_img][2] {feature, world row} with d_nmatches [n_frames], d_final
 * [n_frames][cap_per_img] u8, d_verdict [n_frames] (RS_SV_*), d_pose_out [n_frames][12] f64, d_best (optional, needed where a
 * merged row occurs), d_skip [n_frames] u32 (optional, non-zero: leave the slot out).  obs_room >= n_obs + split_room + n_frames *
 * cap_per_img and lm_room >= n_landmarks + split_room + n_frames * cap_per_img, else AKZ_E_INVALID: no kernel can overflow.
 * A slot is accepted iff its verdict is RS_SV_OK, it is not skipped and it is valid: count and d_nmatches[f] <= cap_per_img and
 * every final match (d_final != 0) names a feature below the count, once, and a row below min(n_world, n_landmarks) or the merged
 * row n_world + f * cap_per_img + feature of its own slot with best[0] != best[1] both below n_landmarks.  A merged match
 * (a, b) is applied iff no other final match of an accepted slot of the call names a or b; else it is demoted to a match of a.
 * Outputs: d_obs_start_out [lm_room + 1], d_obs_out [obs_room][2].  Keys are stable.  Row l < n_landmarks: empty if l is the b of
 * an applied merge; else its old list, the old list of the b merged into it, the new observations {ik[f], feature} in ascending
 * slot order.  Row n_landmarks + k, k < min(*d_split_count, split_room): the k-th split observation.  Then, for the accepted
 * slots in slot order, one row {ik[f], j} for every feature j below the count that is in no final match, ascending (add_landmark).
 * Every start from there to lm_room equals the total: the rows beyond are empty.  d_obs_out behind the total is not written.
 * d_counts_out [RS_AV_COUNTS] u32.  d_landmarks_out [n_blocks][cap_per_img] u32, every word written: the key of the row whose
 * list holds {block, feature} (the lowest, where a broken table lists a feature twice), 0xFFFFFFFF for none — what
 * hm_best_of_views_batch_device reads.  d_obs_counts_out [lm_room] u32: the row lengths
 * (hm_landmark_matches_ordered_batch_device's d_obs_counts).  d_poses [n_blocks][12] f64, in place: row ik[f] = d_pose_out[f] for
 * the accepted slots.  d_frame_verdict [n_frames] u32 (RS_AV_*), d_stats [n_frames][RS_AV_STATS] u32, d_call_verdict [1] u32:
 * RS_AV_OK, or RS_AV_BAD_TABLE for a table whose starts do not ascend inside [0, n_obs] — no slot is accepted then and the
 * outputs describe an empty table.  A stage behind may take (lm_room, obs_room) as its (n_landmarks, n_obs) without waiting for
 * d_counts_out: the empty rows are RS_TRI_TOO_FEW / RS_OF_SINGLE there.  Enqueues on rs_stream() after stream_to_wait (may be
 * NULL) and returns; allocates nothing beyond growing the context's scratch. */
int32_t rs_add_views_device(rs_ctx* ctx, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t n_world,
                            const void* d_split, const void* d_split_count, uint32_t split_room, uint32_t cap_per_img, uint32_t n_blocks,
                            const uint32_t* ik, uint32_t n_frames, const void* d_counts, const void* d_matches, const void* d_nmatches,
                            const void* d_final, const void* d_verdict, const void* d_pose_out, const void* d_best, const void* d_skip,
                            uint32_t obs_room, uint32_t lm_room, void* d_poses, void* d_obs_start_out, void* d_obs_out, void* d_counts_out,
                            void* d_landmarks_out, void* d_obs_counts_out, void* d_frame_verdict, void* d_stats, void* d_call_verdict,
                            void* stream_to_wait);
/* ---- a reconstruction repacked on the device: views removed, the table compacted, rows and blocks renumbered ----
 * VSlamData::remove_view (cv-sfm/src/lib.rs:517-546) for any set of views at once — what apply_bundle_adjust's removed_views
 * (:502-515), incorporate_reconstruction (:1880-1884) and try_merge_reconstructions (:2147) ask for — and the compaction the
 * out-of-place generations of rs_add_views_device never do: tombstones, rows that lost every observation and the empty tail
 * are dropped, rows and blocks renumbered.  A valid table has at most one row per feature of a kept view, so a repacked table
 * always fits n_blocks_out * cap_per_img rows and observations, whatever its history.  Integer data movement; the decisions
 * are include/akz_repack_math.h (compiled for the device and, by the tests, for the host: equal byte for byte), whose head
 * lists the departures from the reference.
 * The block map d_block_map [n_blocks] u32: entry b is the new block of old block b, or 0xFFFFFFFF when the view is removed.
 * NULL is the identity, and then n_blocks_out == n_blocks (else AKZ_E_INVALID).  A map is valid iff every entry is 0xFFFFFFFF
 * or below n_blocks_out and no two blocks share a target; that is checked on the device (a reference count per target). */
enum {
    RS_RP_OK = 0,
    RS_RP_BAD_TABLE = 1,       /* the starts do not ascend inside [0, n_obs], or d_recon_start does not inside [0, n_landmarks] */
    RS_RP_BAD_INDEX = 2,       /* an observation of a row names a block >= n_blocks, or a kept one a feature >= cap_per_img */
    RS_RP_BAD_MAP = 3,         /* the map is not valid */
    RS_RP_NO_ROOM = 4,         /* the kept rows exceed lm_room or the kept observations obs_room; d_counts_out holds the true numbers */
    /* d_counts_out words (u32): */
    RS_RP_C_ROWS = 0,          /* rows kept */
    RS_RP_C_OBSERVATIONS = 1,  /* observations kept */
    RS_RP_C_EMPTY_DROPPED = 2, /* empty rows dropped */
    RS_RP_C_ROWS_DROPPED = 3,  /* rows dropped because every observation was in a removed view */
    RS_RP_C_OBS_DROPPED = 4,   /* observations dropped */
    RS_RP_COUNTS = 5
};
/* The next generation of the table without the removed views, out of place.  Inputs: the table as
 * rs_triangulate_landmarks_device takes it (d_obs_start [n_landmarks + 1], d_obs [n_obs][2] {block, feature}; the rows'
 * observations are the table's, whatever lies behind d_obs_start[n_landmarks] is not read), the map, the optional row ranges of
 * the reconstructions d_recon_start [n_recons + 1] (NULL with n_recons 0 for none), and the rooms of the outputs — they may be
 * smaller than the input, and that is the point.  An observation {b, j} is kept iff map[b] != 0xFFFFFFFF; a row is kept iff
 * it keeps an observation.  Kept rows leave in ascending old key: the new key is the number of kept rows below.  A row's
 * kept observations stay in order, their block replaced by map[b].
 * Outputs, in rs_add_views_device's shapes: d_obs_start_out [lm_room + 1] (every start from the kept rows to lm_room equals
 * the total), d_obs_out [obs_room][2] (not written behind the total), d_obs_counts_out [lm_room] (0 behind the kept rows),
 * d_landmarks_out [n_blocks_out][cap_per_img], every word written: the new key of the row that lists {block, feature} (the
 * lowest, where a broken table lists a feature twice), 0xFFFFFFFF for none; d_key_out [n_landmarks]: the new key of every old
 * row, 0xFFFFFFFF for a dropped one; d_recon_start_out [n_recons + 1]: the kept rows with old key below d_recon_start[r];
 * d_counts_out [RS_RP_COUNTS]; d_call_verdict [1] (RS_RP_*; where several apply: table, map, index, room in that order).
 * On any verdict but RS_RP_OK the outputs describe an empty table: every start 0, every count 0, every map word and key
 * 0xFFFFFFFF, every range start 0, d_obs_out untouched; d_counts_out is 0 unless the verdict is RS_RP_NO_ROOM.  Nothing is
 * read or written out of bounds, and the caller still holds the old generation.  An output that overlaps an input:
 * AKZ_E_INVALID; so are cap_per_img or n_blocks 0 and lm_room 0xFFFFFFFF.  Enqueues on rs_stream() after stream_to_wait (may be
 * NULL) and returns; allocates nothing beyond growing the context's scratch. */
int32_t rs_repack_table_device(rs_ctx* ctx, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks,
                               uint32_t cap_per_img, uint32_t n_blocks, const void* d_block_map, uint32_t n_blocks_out,
                               const void* d_recon_start, uint32_t n_recons, uint32_t obs_room, uint32_t lm_room, void* d_obs_start_out,
                               void* d_obs_out, void* d_obs_counts_out, void* d_landmarks_out, void* d_key_out, void* d_recon_start_out,
                               void* d_counts_out, void* d_call_verdict, void* stream_to_wait);
/* A per-block pool moved through the map: row map[b] of d_dst [n_blocks_out][row_bytes] is row b of d_src
 * [n_blocks][row_bytes] for every kept b, every other row of d_dst is zero: every byte is written.  Keypoints, counts, poses,
 * colours, descriptors, an old d_landmarks_out all move this way.  row_bytes is a multiple of 4 and every pointer 4-byte aligned (else AKZ_E_INVALID); 16-byte
 * accesses where row_bytes and both pointers allow.  d_verdict [1] u32: RS_RP_OK, or RS_RP_BAD_MAP for a map that is not
 * valid — d_dst is all zeros then.  d_src and d_dst may not overlap (AKZ_E_INVALID).  rs_stream(), as above. */
int32_t rs_gather_blocks_device(rs_ctx* ctx, const void* d_src, void* d_dst, uint32_t row_bytes, uint32_t n_blocks, const void* d_block_map,
                                uint32_t n_blocks_out, void* d_verdict, void* stream_to_wait);
/* remove_view's retain over the three-view constraints (lib.rs:541-543), ordered and out of place: d_views [n_constraints][3],
 * d_constraint_poses [n_constraints][2][12] f64 and d_constraint_verdict [n_constraints] as rs_pose_graph_edges_device takes
 * them.  A constraint is kept iff all three of its views are kept (a view >= n_blocks or a map entry that names no block of the
 * output drops it too; the map's validity is rs_repack_table_device's to judge).  The kept constraints leave in order with their
 * views mapped, poses and verdicts moving along, into the same three arrays with room n_constraints; d_count [1] u32.  Behind
 * the count the views are 0xFFFFFFFF, the verdict RS_TVC_BAD_INDEX and the poses 0, so that a caller can pass the room on as
 * n_constraints without reading the count: rs_pose_graph_edges_device gives such a triple zero edges,
 * rs_pose_graph_rows_device leaves it out of the rows (its flag word then reads 1), the relaxation never meets it.  Optional
 * d_start [n_ranges + 1] u32, ranges of constraints (NULL with n_ranges 0 for none): d_start_out[r] = the kept constraints
 * below min(d_start[r], n_constraints).  One workgroup-scan launch on rs_stream(), as above. */
int32_t rs_repack_constraints_device(rs_ctx* ctx, const void* d_views, const void* d_constraint_poses, const void* d_constraint_verdict,
                                     uint32_t n_constraints, const void* d_block_map, uint32_t n_blocks, uint32_t n_blocks_out,
                                     const void* d_start, uint32_t n_ranges, void* d_views_out, void* d_constraint_poses_out,
                                     void* d_constraint_verdict_out, void* d_count, void* d_start_out, void* stream_to_wait);
/* ---- two reconstructions become one on the device: the landmark map of a bridging frame, incorporate, normalise ----
 * cv-sfm's loop closure between reconstructions (VSlam::try_merge_reconstructions, cv-sfm/src/lib.rs:2116-2193;
 * incorporate_reconstruction, lib.rs:1817-1887) and normalize_reconstruction (lib.rs:2241-2283) over the tables
 * rs_add_views_device writes.  The decisions and the pose arithmetic are include/akz_reconstruction_merge_math.h (compiled for
 * the device and, by the tests, for the host: equal byte for byte), whose head lists the departures from the reference. */
enum {
    RS_IR_OK = 0,
    RS_IR_BAD_TABLE = 1,       /* either table's starts do not ascend inside its n_obs */
    RS_IR_BAD_INDEX = 2,       /* a kept source observation names a feature >= cap_per_img */
    RS_IR_SHARED_BLOCK = 3,    /* a kept source observation names a block the destination table names too */
    /* d_counts_out words (u32): */
    RS_IR_C_ROWS = 0,          /* rows filled */
    RS_IR_C_OBSERVATIONS = 1,  /* observations filled */
    RS_IR_C_APPLIED = 2,       /* map entries applied */
    RS_IR_C_DEMOTED = 3,       /* map entries demoted */
    RS_IR_C_NEW_ROWS = 4,      /* rows added behind the destination's */
    RS_IR_C_DROPPED = 5,       /* source observations dropped (the bridging frame's, the skipped views') */
    RS_IR_COUNTS = 6,
    RS_NR_OK = 0,
    RS_NR_NOT_NORMAL = 1,      /* the mean distance is zero, subnormal, infinite or NaN (no robust point at all): nothing is written */
    RS_NR_BAD_INDEX = 2        /* a view block >= n_blocks or the first view's count above cap_per_img: nothing is written */
};
/* The map of lib.rs:2159-2170 for the bridging frame, slot `slot` of a refinement call over the DESTINATION table: d_matches
 * [..][cap_per_img][2], d_nmatches, d_final [..][cap_per_img] u8 and the optional d_best with n_world, as rs_add_views_device
 * takes them; d_counts [n_blocks] u32; d_src_landmarks [n_blocks][cap_per_img] u32 the SOURCE reconstruction's per-feature
 * landmark map (an earlier d_landmarks_out); bridge_block < n_blocks (else AKZ_E_INVALID) the frame's keypoint block.
 * d_map [cap_per_img][2] u32 {source landmark, destination landmark}, d_map_count [1] u32: one entry per final match of the slot
 * that names something under rs_add_views_device's rules (the destination of a merged match is best[0], the reference's
 * dest_landmarks[0]) and whose feature has a source landmark (not 0xFFFFFFFF), in ascending feature order; a feature in two
 * final matches takes the first.  A slot whose count or d_nmatches is above cap_per_img gives an empty map.  Entries behind the
 * count are not written.  One launch of one workgroup on rs_stream() after stream_to_wait (may be NULL); returns after
 * enqueueing; allocates nothing beyond growing the context's scratch. */
int32_t rs_merge_map_device(rs_ctx* ctx, const void* d_matches, const void* d_nmatches, const void* d_final, const void* d_best, uint32_t n_world,
                            uint32_t n_dst_landmarks, uint32_t cap_per_img, uint32_t slot, const void* d_counts, const void* d_src_landmarks,
                            uint32_t n_blocks, uint32_t bridge_block, void* d_map, void* d_map_count, void* stream_to_wait);
/* incorporate_reconstruction, out of place.  The destination table (d_dst_start [n_dst_landmarks + 1], d_dst_obs [n_dst_obs][2])
 * is the table after the bridging frame's add_views; the source table is given the same way; d_map [map_room][2] with its length
 * d_map_count [1] on the device (the first min(*d_map_count, map_room) entries count).  src_blocks [n_src_views] is a host list
 * of distinct blocks below n_blocks that does not hold bridge_block (else AKZ_E_INVALID): the source's other views.  d_src_pose
 * [12] f64 is the bridging frame's pose in the source, copied before add_views overwrote that row of d_poses.  d_skip
 * [n_src_views] u32 (optional, non-zero: the view is left out).  obs_room >= n_dst_obs + n_src_obs and lm_room >=
 * n_dst_landmarks + n_src_landmarks, and no output may overlap an input table or the map: else AKZ_E_INVALID.
 * A source observation is kept iff its block is in src_blocks and not skipped (the bridging frame's are dropped: the reference
 * removes that view from the source first).  A map entry is applied iff it names a row of each table and no other entry names
 * its source landmark and none its destination landmark; else it is demoted and its source landmark is unmapped.  Outputs, in
 * rs_add_views_device's shapes: row l < n_dst_landmarks is its old list, then the kept observations of the source landmark
 * mapped to it in source order; the unmapped source landmarks with a kept observation become rows n_dst_landmarks + k in
 * ascending source key; every start from there to lm_room equals the total.  d_counts_out [RS_IR_COUNTS], d_landmarks_out
 * [n_blocks][cap_per_img] every word written, d_obs_counts_out [lm_room], d_src_key_out [n_src_landmarks] the destination key of
 * every source landmark or 0xFFFFFFFF, d_call_verdict [1] (RS_IR_*).  d_poses [n_blocks][12] f64 in place: with T =
 * inverse(d_src_pose) * d_poses[bridge_block], d_poses[b] = d_poses[b] * T for every kept source view b.  On a verdict other
 * than RS_IR_OK the outputs describe the destination table unchanged (a destination whose own starts are broken: as many
 * empty rows), every source key is 0xFFFFFFFF and the poses are untouched.  Enqueues on rs_stream() after stream_to_wait (may be
 * NULL) and returns; allocates nothing beyond growing the context's scratch. */
int32_t rs_incorporate_reconstruction_device(rs_ctx* ctx, const void* d_dst_start, const void* d_dst_obs, uint32_t n_dst_obs,
                                             uint32_t n_dst_landmarks, const void* d_src_start, const void* d_src_obs, uint32_t n_src_obs,
                                             uint32_t n_src_landmarks, const void* d_map, const void* d_map_count, uint32_t map_room,
                                             uint32_t cap_per_img, uint32_t n_blocks, const uint32_t* src_blocks, uint32_t n_src_views,
                                             uint32_t bridge_block, const void* d_src_pose, const void* d_skip, uint32_t obs_room,
                                             uint32_t lm_room, void* d_poses, void* d_obs_start_out, void* d_obs_out, void* d_counts_out,
                                             void* d_landmarks_out, void* d_obs_counts_out, void* d_src_key_out, void* d_call_verdict,
                                             void* stream_to_wait);
/* normalize_reconstruction for one reconstruction: view_blocks [n_views] a host list of distinct blocks (n_views >= 1, else
 * AKZ_E_INVALID), the first the reference's first view; d_counts [n_blocks], d_landmarks [n_blocks][cap_per_img] (a
 * d_landmarks_out), d_world [n_world][4] f64.  The mean runs over the first view's features j < count whose landmark is below
 * n_world and whose world row has a Euclidean point (w > 0): |(pose * point).xyz / w|, summed in include/akz_sum_order.h's
 * order for 256 threads and divided by the count.  If it is a normal number every listed view's pose becomes pose *
 * inverse(first) with its translation times 1 / mean, and the translations of d_constraint_poses [n_constraints][2][12] f64
 * (optional) are multiplied by the same factor, both in place; else nothing but d_stats and d_verdict is written.  d_stats [2]
 * f64 {mean, count}, d_verdict [1] u32 (RS_NR_*).  One launch of one workgroup of 256 on rs_stream() after stream_to_wait (may
 * be NULL); returns after enqueueing; allocates nothing beyond growing the context's scratch. */
int32_t rs_normalize_reconstruction_device(rs_ctx* ctx, const uint32_t* view_blocks, uint32_t n_views, const void* d_counts,
                                           const void* d_landmarks, uint32_t cap_per_img, uint32_t n_blocks, const void* d_world,
                                           uint32_t n_world, void* d_poses, void* d_constraint_poses, uint32_t n_constraints, void* d_stats,
                                           void* d_verdict, void* stream_to_wait);
/* ---- a reconstruction starts on the device: the join of the pair lists, add_reconstruction ----
 * The two integer steps of cv-sfm's try_init around rs_three_view_init_batch_device: the join and the shuffle of
 * VSlam::init_reconstruction (cv-sfm/src/lib.rs:992-999, 1190-1191, 1216, 1234) in front of it, VSlamData::add_reconstruction
 * (lib.rs:377-427, with add_view / add_landmark, lib.rs:432-500) behind it, so that two-view consensus -> join -> bootstrap -> new
 * reconstruction -> world table -> rs_optimize_reconstruction_batch_device runs on rs_stream() without a host step.  The
 * decisions are include/akz_bootstrap_table_math.h (compiled for the device and, by the tests, for the host: equal byte for
 * byte), whose head lists the departures from the reference. */
enum {
    RS_JP_OK = 0,
    RS_JP_NO_MODEL = 1,        /* d_best_id of either slot is 0xFFFFFFFF */
    RS_JP_FEW_INLIERS = 2,     /* an inlier list shorter than two_view_minimum_robust_matches (lib.rs:1421) */
    RS_JP_BAD_INDEX = 3,       /* a count above cap_per_img, an inlier index not below the slot's d_npairs, or a feature not below
                                * cap_per_img: nothing is read out of bounds */
    RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES = 256,   /* cv-sfm/src/settings.rs:393-395 */
    RS_JP_MAX_FEATURES = 9216, /* cap_per_img at the most (RS_TV_MAX_COMMON: the bootstrap takes no more; a scene's two maps live in
                                * LDS): AKZ_E_TOO_LARGE beyond */
    RS_AR_OK = 0,
    RS_AR_NOT_ACCEPTED = 1,    /* the scene's bootstrap verdict is not RS_TV_OK, d_skip names it, or the call was refused */
    RS_AR_BAD_INDEX = 2,       /* two of its frames are one block, one of its six counts is above cap_per_img, an accepted match names
                                * a feature not below its block's count, or a feature of one view occurs in two accepted matches:
                                * the scene is refused alone */
    RS_AR_TAKEN = 3,           /* an earlier accepted scene of the call names one of its three source frames */
    RS_AR_BAD_TABLE = 4,       /* d_call_verdict only */
    /* d_stats words (u32) of a scene, all 0 unless it is accepted: */
    RS_AR_S_TRIPLES = 0,       /* accepted triples */
    RS_AR_S_FIRST = 1,         /* accepted first-only pairs */
    RS_AR_S_SECOND = 2,        /* accepted second-only pairs */
    RS_AR_S_LANDMARKS = 3,     /* rows of the new reconstruction */
    RS_AR_STATS = 4,
    RS_AR_COUNTS = 4           /* d_counts_out: {rows filled, observations filled, reconstructions, scenes accepted} */
};
/* The join.  Scene s < n_scenes names two slots of one rs_essential_arrsac_batch_device call run with the centre frame as side a:
 * slot_first[s] and slot_second[s] (host lists, below n_slots, else AKZ_E_INVALID).  Inputs as that call and the matcher left
 * them: d_pairs [n_slots][cap_per_img][2], d_npairs, d_inliers [n_slots][cap_per_img], d_n_inliers, d_best_id [n_slots], d_pose
 * [n_slots][12] f64.  A slot's list is d_pairs[d_inliers[i]] = {centre, other feature} in inlier order.  Outputs, indexed by
 * scene, are what rs_three_view_init_batch_device reads: d_triples [n_scenes][cap_per_img][3] {centre, first, second} with
 * d_ntriples — one per entry of the first list whose centre feature the second list has, in the order of the first list,
 * duplicates included, the second feature from the LAST entry of the second list with that centre; d_first_only / d_second_only
 * [n_scenes][cap_per_img][2] with d_nfirst / d_nsecond — the entries of a list whose centre feature the other list lacks, in the
 * order of their own list; d_pose_first / d_pose_second [n_scenes][12] f64 the slots' poses (always copied); d_verdict [n_scenes]
 * u32 (RS_JP_*).  A scene that is not RS_JP_OK gets three zero counts — the bootstrap refuses it by itself — and its lists are
 * not written.  With RS_BATCH_SHUFFLE in flags (no other bit, else AKZ_E_INVALID) the triples are shuffled by that flag's rule
 * with the scene seed seed + 0x9E3779B97F4A7C15 * s; it needs cap_per_img <= 8192 (AKZ_E_TOO_LARGE).  Entries behind a count are
 * not written.  n_scenes <= 65535.  One launch, one workgroup per scene, on rs_stream() after stream_to_wait (may be NULL);
 * returns after enqueueing; allocates nothing beyond growing the context's scratch. */
int32_t rs_join_pairs_batch_device(rs_ctx* ctx, const void* d_pairs, const void* d_npairs, const void* d_inliers, const void* d_n_inliers,
                                   const void* d_best_id, const void* d_pose, uint32_t n_slots, uint32_t cap_per_img,
                                   const uint32_t* slot_first, const uint32_t* slot_second, uint32_t n_scenes,
                                   uint32_t two_view_minimum_robust_matches, uint32_t flags, uint64_t seed, void* d_triples,
                                   void* d_ntriples, void* d_first_only, void* d_nfirst, void* d_second_only, void* d_nsecond,
                                   void* d_pose_first, void* d_pose_second, void* d_verdict, void* stream_to_wait);
/* add_reconstruction for the accepted scenes of an rs_three_view_init_batch_device call, out of place.
 * Inputs: that call's lists, masks, d_pose_out [n_scenes][2][12] and d_verdict where it left them; ic / i_first / i_second the
 * host lists of source blocks (below n_src_blocks, else AKZ_E_INVALID) of d_kps [n_src_blocks][cap_per_img] akz_keypoint with
 * d_counts [n_src_blocks] u32; d_skip [n_scenes] u32 (optional, non-zero: leave the scene out); an optional existing table
 * (d_obs_start [n_landmarks + 1], d_obs [n_obs][2]) with the ranges of its reconstructions d_recon_start / d_view_start
 * [n_recons + 1] u32 over its rows and its views — all NULL / 0 for none.  The destination pool: d_kps_dst [n_blocks][cap_per_img],
 * d_counts_dst [n_blocks], d_poses [n_blocks][12] f64.  Scene s is reconstruction n_recons + s and owns the views (destination
 * blocks) view_base + 3 s .. + 3 in the order {centre, first, second}.
 * Refused before anything is enqueued (AKZ_E_INVALID): view_base + 3 n_scenes > n_blocks; d_kps_dst partially overlaps d_kps;
 * d_kps_dst == d_kps and the destination range holds a named source block; lm_room < n_landmarks + 3 n_scenes cap_per_img or
 * obs_room < n_obs + 3 n_scenes cap_per_img; an output table or range array that overlaps the input table or its ranges.
 * An accepted match is a triple with d_combined != 0, a first-only pair with d_first_ok != 0, a second-only pair with
 * d_second_ok != 0.  In scene order, scene s is accepted iff its verdict is RS_TV_OK, it is not skipped, it is valid
 * (RS_AR_BAD_INDEX otherwise) and no earlier accepted scene of the call names one of its three source frames (RS_AR_TAKEN).
 * Outputs in rs_add_views_device's shapes: d_obs_start_out [lm_room + 1], d_obs_out [obs_room][2], d_obs_counts_out [lm_room],
 * d_counts_out [RS_AR_COUNTS], d_landmarks_out [n_blocks][cap_per_img] every word written (global keys, 0xFFFFFFFF for none).  The
 * old rows keep their keys and lists.  Behind them the rows of the accepted scenes in scene order: row j for every centre
 * feature j below its count = {centre view, j}, then {first view, f} if an accepted match maps f to j, then {second view, s}
 * likewise; one row for every first-frame feature in no accepted match, ascending; one for every second-frame feature in none.  A
 * refused scene owns an empty row range (and three views no accepted constraint names).  Every start behind the total equals
 * the total; d_obs_out behind it is not written.  d_recon_start_out / d_view_start_out [n_recons + n_scenes + 1]: the old ranges,
 * then the scenes'.  For the accepted scenes the three keypoint blocks and counts are copied to their views and d_poses gets
 * the identity, d_pose_out[s][0] and d_pose_out[s][1].  The first ThreeViewConstraint of every scene, as
 * rs_pose_graph_edges_device and rs_pose_graph_rows_device take it: d_views_out [n_scenes][3], d_constraint_poses_out
 * [n_scenes][24] f64 (accepted scenes only), d_constraint_verdict_out [n_scenes] u32: RS_TVC_OK for an accepted scene, else
 * RS_CV_NOT_RECORDED.  d_frame_verdict [n_scenes] u32 (RS_AR_*), d_stats [n_scenes][RS_AR_STATS] u32, d_call_verdict [1] u32:
 * RS_AR_OK, or RS_AR_BAD_TABLE for an existing table whose starts do not ascend inside [0, n_obs], whose reconstruction ranges do
 * not ascend up to n_landmarks, or whose view ranges do not ascend up to view_base — no scene is accepted then and the outputs
 * describe the old table unchanged, word for word, every new range empty.  n_scenes <= 65535.  Enqueues on rs_stream() after
 * stream_to_wait (may be NULL) and returns; allocates nothing beyond growing the context's scratch. */
int32_t rs_add_reconstruction_batch_device(rs_ctx* ctx, const void* d_triples, const void* d_ntriples, const void* d_first_only,
                                           const void* d_nfirst, const void* d_second_only, const void* d_nsecond, const void* d_combined,
                                           const void* d_first_ok, const void* d_second_ok, const void* d_pose_out, const void* d_verdict,
                                           const uint32_t* ic, const uint32_t* i_first, const uint32_t* i_second, uint32_t n_scenes,
                                           const void* d_kps, const void* d_counts, uint32_t n_src_blocks, uint32_t cap_per_img,
                                           const void* d_skip, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
                                           uint32_t n_landmarks, const void* d_recon_start, const void* d_view_start, uint32_t n_recons,
                                           void* d_kps_dst, void* d_counts_dst, void* d_poses, uint32_t n_blocks, uint32_t view_base,
                                           uint32_t obs_room, uint32_t lm_room, void* d_obs_start_out, void* d_obs_out,
                                           void* d_obs_counts_out, void* d_counts_out, void* d_landmarks_out, void* d_recon_start_out,
                                           void* d_view_start_out, void* d_views_out, void* d_constraint_poses_out,
                                           void* d_constraint_verdict_out, void* d_frame_verdict, void* d_stats, void* d_call_verdict,
                                           void* stream_to_wait);
/* ---- a reconstruction leaves the device: the coloured point cloud and the cameras' frusta of export_reconstruction ----
 * VSlam::export_reconstruction (cv-sfm/src/lib.rs:2285-2340) with export.rs: everything but the text of the file.  The decisions
 * and the arithmetic are include/akz_export_math.h (compiled for the device and, by the tests, for the host: equal byte for
 * byte), whose head lists the departures from the reference. */
enum {
    RS_EX_OK = 0,
    RS_EX_OVERFLOW = 1,        /* more points than `room`: the first `room` are written, nothing lands behind them */
    RS_EX_BAD_TABLE = 2,       /* d_obs_start[0] != 0, or the starts do not ascend inside [0, n_obs]: no point is written */
    /* d_counts_out words (u32): */
    RS_EX_C_POINTS = 0,        /* points exported: the true number, even beyond `room` */
    RS_EX_C_NO_POINT = 1,      /* rows skipped for w < 0 (the triangulation's "none") */
    RS_EX_C_INFINITE = 2,      /* rows skipped for w == 0 (a NaN among them) */
    RS_EX_C_BAD_ROWS = 3,      /* rows with w > 0 skipped for their list: empty, outside the table, a first entry outside the colours */
    RS_EX_COUNTS = 4,
    RS_EX_CAMERA_WORDS = 10,   /* a row of d_cameras: centre [3], up [3], forward [3], focal length */
    RS_EX_CAMERA_VERTICES = 5  /* the vertices of a camera: the centre, then up-right, up-left, down-left, down-right */
};
/* d_world [n_world][4] f64 (rs_triangulate_landmarks_device's), the landmark table (d_obs_start [n_landmarks + 1], d_obs
 * [n_obs][2] {block, feature}), d_colors [n_blocks][cap_per_img][3] u8 (akz_sample_colors_batch_device's), view_blocks [n_views] a
 * host list of distinct blocks below n_blocks with n_views >= 1 (else AKZ_E_INVALID), d_counts [n_blocks] u32, d_landmarks
 * [n_blocks][cap_per_img] u32 (a d_landmarks_out), d_poses [n_blocks][12] f64 WorldToCamera.
 * Outputs, in the order export.rs adds the vertices: d_xyz [5 * n_views + room][3] f64 and d_rgb [5 * n_views + room][3] u8 —
 * vertices [5 v, 5 v + 5) are camera v's (colour {255, 0, 255}), vertex 5 * n_views + k is point k; d_key [room] u32 the landmark
 * of point k; d_cameras [n_views][RS_EX_CAMERA_WORDS] f64; d_counts_out [RS_EX_COUNTS] u32; d_verdict [1] u32 (RS_EX_*).
 * Row l < n_world is a point iff w > 0: x / w, y / w, z / w, coloured by the first entry of its observation list; the points
 * ascend with l.  A row with w > 0 whose list is empty or leaves [0, n_obs] (a row at or behind n_landmarks has none), or whose
 * first entry names a block >= n_blocks or a feature >= cap_per_img, is skipped alone and counted.  Points at or behind `room`
 * are counted and not written.  A camera's focal length is 0.01 times the mean distance of the view's features j < min(count,
 * cap_per_img) whose landmark is below n_world and has a Euclidean point, summed in include/akz_sum_order.h's order for 256
 * threads; a mean over nothing is 0.  On RS_EX_BAD_TABLE the counters are 0 and the cameras are still written.  Nothing is read
 * out of bounds.  Refused from the arguments alone, before the context is looked at: a null pointer, cap_per_img, n_blocks or
 * n_views of 0, a repeated or out-of-range block, an output that overlaps an input (AKZ_E_INVALID), sizes that overflow 32-bit
 * arithmetic (AKZ_E_TOO_LARGE).  Five launches on rs_stream() after stream_to_wait (may be NULL); returns after enqueueing;
 * allocates nothing beyond growing the context's scratch. */
int32_t rs_export_reconstruction_device(rs_ctx* ctx, const void* d_world, uint32_t n_world, const void* d_obs_start, const void* d_obs,
                                        uint32_t n_obs, uint32_t n_landmarks, const void* d_colors, const uint32_t* view_blocks,
                                        uint32_t n_views, const void* d_counts, const void* d_landmarks, uint32_t cap_per_img,
                                        uint32_t n_blocks, const void* d_poses, uint32_t room, void* d_xyz, void* d_rgb, void* d_key,
                                        void* d_cameras, void* d_counts_out, void* d_verdict, void* stream_to_wait);
/* The file export.rs writes, from host arrays (no GPU): an ASCII .ply with the comment "Exported from rust-cv/vslam-sandbox",
 * `element vertex` (double x y z, uchar red green blue) and, with camera_faces != 0, `element face` (property list uchar int
 * vertex_index).  xyz [n_vertices][3] f64 and rgb [n_vertices][3] u8 in the given order; the first 5 * n_cameras vertices are
 * the cameras' (more than n_vertices: AKZ_E_INVALID), and camera v with b = 5 v gets the triangles (b, b + 4, b + 1), (b, b + 1,
 * b + 2), (b, b + 2, b + 3), (b, b + 3, b + 4).  Numbers are written with %.17g: a reader gets the same f64 bits back.  A file
 * that cannot be written: AKZ_E_INVALID. */
int32_t rs_write_ply(const char* path, const double* xyz, const uint8_t* rgb, uint32_t n_vertices, uint32_t n_cameras, int32_t camera_faces);
int32_t rs_sync(rs_ctx* ctx);
void* rs_stream(rs_ctx* ctx);
/* parity tap: match count, calibrated bearings [n][3] (a, b) and scoring order [n] of scene `scene` of the last batched
 * call (any of the three pointers may be NULL) */
int32_t rs_debug_scene(rs_ctx* ctx, uint32_t scene, uint32_t* n, double* bearings_a, double* bearings_b, uint32_t* order,
                       uint32_t cap);
/* the same after rs_p3p_arrsac_batch_device: bearings [n][3], world points [n][4] */
int32_t rs_debug_scene_world(rs_ctx* ctx, uint32_t scene, uint32_t* n, double* bearings, double* world, uint32_t* order,
                             uint32_t cap);

/* ---- the exchange step of the frame-sharded front-end ----
 * Frames shard over the GPUs of a node as frame g -> rank g mod N (extraction is stateless per frame: akaze::Akaze is
 * Copy, akaze/src/lib.rs:108).  A new frame is matched against its recent predecessors g-1 .. g-k (cv-sfm/src/lib.rs:
 * 1462-1486; tracking_recent_frames = 32, cv-sfm/src/settings.rs:449-450), which live on the other ranks: the
 * descriptor blocks a rank has extracted — fixed capacity, [n_frames][cap_per_img][64] bytes + [n_frames] u32 counts,
 * exactly akz_extract_batch_device's outputs — travel by a ring shift (k = 1: a rank needs its predecessor's block) or
 * by an all-gather (k >= N - 1).  RCCL directly (ncclSend/ncclRecv/ncclAllGather on akz_comm_stream()), loaded with
 * dlopen("librccl.so.1") on first use.  One process per GPU; rank 0 makes the id, the host application hands it to the
 * other ranks by its own means, every rank creates its communicator.  Calls enqueue and return; they wait for
 * stream_to_wait (the producer of the send rows and last reader of the receive rows; may be NULL), consumers take
 * akz_comm_stream() as their stream_to_wait. */
typedef struct akz_comm akz_comm;
int32_t akz_comm_unique_id(uint8_t* id128);                    /* 128 bytes (ncclUniqueId) */
int32_t akz_comm_create(const uint8_t* id128, int32_t rank, int32_t world, int32_t device, akz_comm** out);
int32_t akz_comm_destroy(akz_comm* comm);
/* this rank's blocks -> rank + 1; the blocks of rank - 1 -> d_recv_descs / d_recv_counts (same shapes) */
int32_t akz_comm_shift_blocks(akz_comm* comm, const void* d_descs, const void* d_counts, uint32_t n_frames, uint32_t cap_per_img,
                              void* d_recv_descs, void* d_recv_counts, void* stream_to_wait);
/* every rank's blocks -> every rank: d_all_descs [world][n_frames][cap_per_img][64], d_all_counts [world][n_frames] */
int32_t akz_comm_allgather_blocks(akz_comm* comm, const void* d_descs, const void* d_counts, uint32_t n_frames, uint32_t cap_per_img,
                                  void* d_all_descs, void* d_all_counts, void* stream_to_wait);
int32_t akz_comm_sync(akz_comm* comm);
void* akz_comm_stream(akz_comm* comm);
int32_t akz_comm_rank(akz_comm* comm);
int32_t akz_comm_world(akz_comm* comm);
/* HIP-event time of the transfers on akz_comm_stream() (their exposed time is what a step loses to them), call and byte
 * counts since the last reset; `enable` switches the brackets on or off for the calls that follow. */
int32_t akz_comm_timing(akz_comm* comm, int32_t enable, double* ms, uint64_t* calls, uint64_t* bytes, int32_t reset);
const char* akz_comm_last_error_string(void);

/* ---- misc ---- */
const char* akz_strerror(int32_t status);
/* hipError_t of the most recent failing HIP call on this thread (0 if none) and its text. */
int32_t akz_last_hip_error(void);
const char* akz_last_hip_error_string(void);
const char* akz_version(void);
/* The ABI number: raised whenever an existing declaration, struct layout or enum value of this header changes.  A pure
 * addition (a new function, struct or enum that leaves every existing one as it was) does not raise it: a binding written
 * against the same number still finds everything it declares.  A binding compares akz_abi_version() of the library it
 * loaded with the AKZ_ABI_VERSION it was written against and refuses to run on a mismatch (cv_amd/_lib.py,
 * rust/akaze-mi355x/src/lib.rs, include/akaze.hpp do). */
#define AKZ_ABI_VERSION 11u
uint32_t akz_abi_version(void);

/* HIP-event timing of the kernel families of a batch (bench.py's roofline objects).  Kernel families (every id but the
 * phase ids below): each launch carries its own start / stop events (hipExtLaunchKernel — the dispatch's begin and end
 * timestamps, the duration rocprofv3's kernel trace reports), so a family's time is the sum of its kernels' own
 * durations whatever else shares the GPU.  Phases (AKZ_T_FED, _SCALE_SPACE, _EXTRACT, _DESCRIBE, _REFINE): an event
 * bracket on the stream, i.e. wall time including waits for the other streams.  akz_timing_enable(ctx, 1) turns both
 * kinds on, 2 the kernel families only (no extra packets in the streams: usable inside a timed region), 0 off.
 * `which` is an AKZ_T_* id;
 * the call returns the milliseconds, launch count and processed units accumulated since akz_timing_reset():
 * units = pixel-frames the launches covered (FED: pixel-steps, the contract's unit; AKZ_T_FED_PASS reports the
 * same launches with units = pixel-frames per launch, i.e. passes over memory). */
enum {
    AKZ_T_FED = 0,        /* k_fed_pair / k_fed_step (calculate_step)                          units: pixel-steps */
    AKZ_T_SCALE_SPACE = 1, /* the whole scale space of a call                                  units: frames */
    AKZ_T_EXTRACT = 2,    /* the whole extract call (closes on the keypoint stream)            units: frames */
    AKZ_T_FRONT0 = 3,     /* level-0 front end: pixels -> blur 1.6 -> Lt[0], {Lx,Ly}           units: pixel-frames */
    AKZ_T_FRONT_SG2 = 4,  /* level front end (blur 1.0, Lflow, {Lx,Ly}) at derivative sigma 2  units: pixel-frames */
    AKZ_T_FRONT_SG3 = 5,
    AKZ_T_FRONT_SG4 = 6,
    AKZ_T_DET_SG2 = 7,    /* second derivatives + determinant + extrema candidates, sigma 2    units: pixel-frames */
    AKZ_T_DET_SG3 = 8,
    AKZ_T_DET_SG4 = 9,
    AKZ_T_CONTRAST = 10,  /* contrast-factor passes                                            units: pixel-frames per pass */
    AKZ_T_DESCRIBE = 11,  /* M-LDB descriptors (keypoint stream)                               units: frames */
    AKZ_T_REFINE = 12,    /* sub-pixel refinement + orientation (keypoint stream)              units: frames */
    AKZ_T_FED_PASS = 13,  /* = AKZ_T_FED with units = pixel-frames per launch */
    AKZ_T_FED_T1 = 14,    /* k_fed_pair<T> launches by T = 1..8 (ids 14..21), units = pixel-frames per launch */
    AKZ_T_FRONT_FED_SG2 = 22, /* fused level front end + first FED launch (k_front_fed), sigma 2..4: ids 22..24,
                               * units = pixel-frames */
    AKZ_T_FRONT_FED_SG3 = 23,
    AKZ_T_FRONT_FED_SG4 = 24,
    AKZ_T_ORIENT_DESCRIBE_K = 25, /* the k_orient_describe launch itself (kernel timer inside the AKZ_T_DESCRIBE phase), units: frames */
    AKZ_T_FRONT_FED_DEEP_SG2 = 26, /* k_front_fed on levels BELOW the first octave (two-patch halo for launches of 5..8 steps; Lflow is */
    AKZ_T_FRONT_FED_DEEP_SG3 = 27, /* written when a later launch of the level reads it), sigma 2..4: ids 26..28, units: pixel-frames */
    AKZ_T_FRONT_FED_DEEP_SG4 = 28,
    AKZ_T_LEVEL_RESIDENT = 29, /* k_level_resident: front end + EVERY FED step of a level that fits one compute unit (octave 3 of a 1080p
                                * pyramid), one launch per level, one workgroup per frame; units: pixel-frames */
    AKZ_T_COUNT = 30
};
int32_t akz_timing_enable(akz_ctx* ctx, int32_t on);
int32_t akz_timing_reset(akz_ctx* ctx);
int32_t akz_timing_get(akz_ctx* ctx, int32_t which, double* ms, uint64_t* launches, uint64_t* units);

#ifdef __cplusplus
}
#endif
#endif /* AKZ_H */
