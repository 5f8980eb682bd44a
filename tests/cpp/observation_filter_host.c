/* The CPU checker of the observation filter: thin exported wrappers around include/akz_observation_filter_math.h, the text
 * cv_amd/csrc/rs_observation_filter.hip compiles for the device.  tests/observation_filter_checker.py has tests/host_build.py
 * build this with the host compiler (its `load`: -O2, no contraction to FMA) into a shared object and loads it with ctypes.
 * The loops around the header (which reconstruction runs, which landmark belongs to it, the scan over the keep flags) restate
 * the kernels' one after another; the arithmetic and every decision on a landmark are the header's. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_observation_filter_math.h"

typedef struct of_camera {   /* rs_camera of include/akz.h */
    double fx, fy, cx, cy, skew, k1;
    int32_t use_k1, reserved;
} of_camera;

#define KP_BYTES 28   /* akz_keypoint: x, y (f32) first */
#define OF_NONE 0xFFFFFFFFu

/* ---- a list handed over as arrays ---- */
typedef struct array_src {
    const double* poses;
    const double* bearings;
} array_src;
static inline int array_fetch(const array_src* s, unsigned i, double* pose, double* b)
{
    for (int k = 0; k < 12; ++k) pose[k] = s->poses[(size_t)12 * i + k];
    for (int k = 0; k < 3; ++k) b[k] = s->bearings[(size_t)3 * i + k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(array_triangulate, array_src, array_fetch)
AKZ_OF_DEFINE_FILTER(array_filter, array_src, array_fetch, array_triangulate)

/* one list: -> state; keep [n], out = {tri_reason, robust, n_split} */
int of_list(const double* poses, const double* bearings, uint32_t n, const akz_of_settings* st, unsigned char* keep, uint32_t* out)
{
    array_src s = {poses, bearings};
    akz_of_result res;
    const int state = array_filter(&s, n, st, keep, &res);
    out[0] = (uint32_t)res.tri_reason; out[1] = res.robust; out[2] = res.n_split;
    return state;
}

/* ---- CSR lists of {block, feature} ---- */
typedef struct list_src {
    const uint32_t* obs;
    const unsigned char* kps;
    const double* poses;
    const of_camera* cam;
    uint32_t s0, cap, n_blocks;
} list_src;
static inline int list_fetch(const list_src* s, unsigned i, double* pose, double* b)
{
    const size_t at = (size_t)s->s0 + i;
    const uint32_t blk = s->obs[2 * at], feat = s->obs[2 * at + 1];
    if (blk >= s->n_blocks || feat >= s->cap) return 0;
    const float* kp = (const float*)(s->kps + ((size_t)blk * s->cap + feat) * KP_BYTES);
    akz_tri_calibrate(&s->cam->fx, s->cam->use_k1, s->cam->k1, kp[0], kp[1], b);
    for (int k = 0; k < 12; ++k) pose[k] = s->poses[(size_t)12 * blk + k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(list_triangulate, list_src, list_fetch)
AKZ_OF_DEFINE_FILTER(list_filter, list_src, list_fetch, list_triangulate)

/* k_of_prepare for reconstruction r: 1 when it may run */
static int recon_ranges_ok(const uint32_t* recon_start, const uint32_t* view_start, uint32_t r, const uint32_t* obs_start, uint32_t n_obs,
                           uint32_t n_landmarks, uint32_t n_blocks)
{
    const uint32_t rs = recon_start[r], re = recon_start[r + 1], vs = view_start[r], ve = view_start[r + 1];
    if (rs > re || re > n_landmarks || vs > ve || ve > n_blocks) return 0;
    for (uint32_t k = 0; k < r; ++k)
        if (recon_start[k] > rs) return 0;
    for (uint32_t l = 0; l < rs; ++l)
        if (obs_start[l] > obs_start[rs]) return 0;
    for (uint32_t l = rs; l < re; ++l)
        if (obs_start[l] > obs_start[l + 1]) return 0;
    return obs_start[re] <= n_obs;
}

/* rs_filter_observations_device on host arrays.  distance (optional) [n_obs] f64: for the observations of a running landmark of
 * three or more with a point, the cosine distance the walk compared; of a running pair, the loss is_bi_landmark_robust compared,
 * at the pair's second observation; NaN-free filler -1 elsewhere.  (A restatement for the tests' band measurement only: the
 * decisions are the header's.) */
int of_filter(const unsigned char* kps, uint32_t cap, uint32_t n_blocks, const double* poses, const of_camera* cam, const uint32_t* obs_start,
              const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, const uint32_t* recon_start, const uint32_t* view_start,
              uint32_t n_recons, const uint32_t* skip, const akz_of_settings* settings, unsigned char* keep, unsigned char* lm_state,
              unsigned char* tri_reason, unsigned char* robust, uint32_t* obs_start_out, uint32_t* obs_out, uint32_t* split_out,
              uint32_t* counts, uint32_t* verdict, uint32_t* stats, double* distance)
{
    uint32_t* lm_recon = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)n_landmarks + 1));
    uint32_t* recon_views = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)n_recons + 1));
    uint32_t* pos = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)n_obs + 1));
    if (!lm_recon || !recon_views || !pos) {
        free(lm_recon); free(recon_views); free(pos);
        return -1;
    }
    for (uint32_t l = 0; l < n_landmarks; ++l) lm_recon[l] = OF_NONE;
    for (uint32_t i = 0; i < n_obs; ++i) keep[i] = 1;
    if (distance)
        for (uint32_t i = 0; i < n_obs; ++i) distance[i] = -1.0;
    for (uint32_t r = 0; r < n_recons; ++r) {
        const int ok = recon_ranges_ok(recon_start, view_start, r, obs_start, n_obs, n_landmarks, n_blocks);
        const int skipped = ok && skip && skip[r] != 0u;
        for (int k = 0; k < AKZ_OF_STATS; ++k) stats[(size_t)AKZ_OF_STATS * r + k] = 0u;
        if (ok) stats[(size_t)AKZ_OF_STATS * r + AKZ_OF_S_LANDMARKS] = recon_start[r + 1] - recon_start[r];
        recon_views[r] = ok ? view_start[r + 1] - view_start[r] : 0u;
        verdict[r] = !ok ? AKZ_OF_BAD_RANGE : skipped ? AKZ_OF_RECON_SKIPPED : AKZ_OF_OK;
        if (ok && !skipped)
            for (uint32_t l = recon_start[r]; l < recon_start[r + 1]; ++l) lm_recon[l] = r;
    }
    for (uint32_t l = 0; l < n_landmarks; ++l) {
        const uint32_t r = lm_recon[l];
        int state = AKZ_OF_SKIPPED;
        akz_of_result res = {AKZ_OF_NO_SOLVE, 0u, 0u};
        if (r != OF_NONE) {
            akz_of_settings st = *settings;
            list_src s = {obs, kps, poses, cam, obs_start[l], cap, n_blocks};
            const uint32_t n = obs_start[l + 1] - obs_start[l];
            uint32_t* w = stats + (size_t)AKZ_OF_STATS * r;
            st.tri.n_views = recon_views[r];
            state = list_filter(&s, n, &st, keep + s.s0, &res);
            w[AKZ_OF_S_ROBUST_BEFORE] += (res.robust & AKZ_OF_ROBUST_BEFORE) ? 1u : 0u;
            w[AKZ_OF_S_ROBUST_AFTER] += (res.robust & AKZ_OF_ROBUST_AFTER) ? 1u : 0u;
            w[AKZ_OF_S_OBS_SPLIT] += res.n_split;
            w[AKZ_OF_S_PAIR_SPLIT] += state == AKZ_OF_PAIR_SPLIT ? 1u : 0u;
            w[AKZ_OF_S_NO_POINT] += state == AKZ_OF_NO_POINT ? 1u : 0u;
            w[AKZ_OF_S_KICKED] += state == AKZ_OF_KICKED ? 1u : 0u;
            if (distance && state != AKZ_OF_BAD_INDEX && n >= 2u) {
                double pose[12], b[3] = {0.0, 0.0, 0.0}, p[4];
                if (n == 2u) {
                    double first[12], inv[12], total[12], b0[3] = {0.0, 0.0, 0.0}, ra[3];
                    list_fetch(&s, 0u, first, b0);
                    list_fetch(&s, 1u, pose, b);
                    akz_tv_pose_inverse(first, inv);
                    akz_tvc_pose_mul(pose, inv, total);
                    akz_tv_rotate(total, b0, ra);
                    const double t[3] = {total[3], total[7], total[11]};
                    distance[s.s0 + 1] = akz_tv_loss(t, ra, b);
                } else if (list_triangulate(&s, n, 0, &st.tri, p) == AKZ_TRI_OK) {
                    for (uint32_t i = 0; i < n; ++i) {
                        list_fetch(&s, i, pose, b);
                        distance[s.s0 + i] = akz_tv_transformed_distance(pose, p, b);
                    }
                }
            }
        }
        lm_state[l] = (unsigned char)state;
        tri_reason[l] = (unsigned char)res.tri_reason;
        robust[l] = (unsigned char)res.robust;
    }
    /* the scan over the table's observations and the two compacted lists */
    const uint32_t filled = obs_start[n_landmarks] < n_obs ? obs_start[n_landmarks] : n_obs;
    uint32_t kept = 0;
    for (uint32_t i = 0; i < filled; ++i) {
        pos[i] = kept;
        uint32_t* row = keep[i] ? obs_out + 2 * (size_t)kept : split_out + 2 * (size_t)(i - kept);
        row[0] = obs[2 * (size_t)i];
        row[1] = obs[2 * (size_t)i + 1];
        kept += keep[i] ? 1u : 0u;
    }
    pos[filled] = kept;
    counts[0] = kept;
    counts[1] = filled - kept;
    for (uint32_t l = 0; l <= n_landmarks; ++l) obs_start_out[l] = pos[obs_start[l] < filled ? obs_start[l] : filled];
    for (uint32_t r = 0; r < n_recons; ++r)
        if (verdict[r] == (uint32_t)AKZ_OF_OK)
            verdict[r] = (uint32_t)akz_of_verdict(stats[(size_t)AKZ_OF_STATS * r + AKZ_OF_S_ROBUST_AFTER], settings->minimum_robust_landmarks);
    free(lm_recon); free(recon_views); free(pos);
    return 0;
}

/* k_or_note of the chain: a reconstruction a stage did not pass stops, its verdict says where */
void of_note(const uint32_t* stage_verdict, uint32_t ok, uint32_t round, uint32_t stage, uint32_t n, uint32_t* stop, uint32_t* verdict)
{
    for (uint32_t r = 0; r < n; ++r) {
        if (stop[r] != 0u || stage_verdict[r] == ok) continue;
        stop[r] = 1u;
        verdict[r] = (1u << 30) | round << 16 | stage << 8 | (stage_verdict[r] & 0xFFu);
    }
}

/* ---- the pieces, for the rule tests ---- */
double of_transformed_distance(const double* pose, const double* point, const double* b) { return akz_tv_transformed_distance(pose, point, b); }
int of_verdict(uint32_t robust_after, uint32_t minimum) { return akz_of_verdict(robust_after, minimum); }
int of_triangulate(const double* poses, const double* bearings, uint32_t n, const akz_tri_settings* st, double* out)
{
    array_src s = {poses, bearings};
    return array_triangulate(&s, n, 0, st, out);
}
void of_calibrate(const of_camera* cam, float x, float y, double* out) { akz_tri_calibrate(&cam->fx, cam->use_k1, cam->k1, x, y, out); }
