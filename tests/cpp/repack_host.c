/* The CPU checker of the repack kernels: the passes of cv_amd/csrc/rs_repack.hip restated one after another around
 * include/akz_repack_math.h, the text the kernels compile for the device.  tests/host_build.py builds this with the host
 * compiler into a shared object.  Every output buffer is produced whole: what the device call does not write is not written
 * here either, so that both sides can start from one fill. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/akz_repack_math.h"

/* the map's validity: a reference count per target (k_rp_count / k_rp_map_check).  inv (or NULL) [n_blocks_out] gets the block
 * of every target.  -1: out of memory. */
static int rp_map_bad(const uint32_t* map, uint32_t n_blocks, uint32_t n_blocks_out, uint32_t* inv)
{
    int bad = 0;
    if (inv) memset(inv, 0xFF, ((size_t)n_blocks_out + 1) * sizeof(uint32_t));
    if (!map) {
        if (inv)
            for (uint32_t b = 0; b < n_blocks_out; ++b) inv[b] = b;
        return 0;
    }
    uint32_t* refs = (uint32_t*)calloc((size_t)n_blocks_out + 1, sizeof(uint32_t));
    if (!refs) return -1;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t m = map[b];
        if (m == AKZ_RP_NONE) continue;
        if (akz_rp_entry_bad(m, n_blocks_out)) bad = 1;
        else if (akz_rp_target_shared(refs[m]++)) bad = 1;
        else if (inv) inv[m] = b;
    }
    free(refs);
    return bad;
}

/* rs_repack_table_device on host arrays (the refusals of the entry point are not restated).  -1: out of memory. */
int rp_table(const uint32_t* obs_start, const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t cap, uint32_t n_blocks,
             const uint32_t* map, uint32_t n_blocks_out, const uint32_t* recon_start, uint32_t n_recons, uint32_t obs_room, uint32_t lm_room,
             uint32_t* obs_start_out, uint32_t* obs_out, uint32_t* obs_counts_out, uint32_t* landmarks_out, uint32_t* key_out,
             uint32_t* recon_start_out, uint32_t* counts_out, uint32_t* call_verdict)
{
    uint32_t* kept = (uint32_t*)calloc((size_t)n_landmarks + 1, sizeof(uint32_t));
    if (!kept) return -1;
    memset(landmarks_out, 0xFF, (size_t)n_blocks_out * cap * sizeof(uint32_t));

    /* k_rp_count */
    int bad_table = 0, bad_index = 0;
    const int bad_map = rp_map_bad(map, n_blocks, n_blocks_out, NULL);
    if (bad_map < 0) {
        free(kept);
        return -1;
    }
    if (recon_start)
        for (uint32_t r = 0; r <= n_recons; ++r) bad_table |= akz_rp_range_bad(recon_start, r, n_recons, n_landmarks);
    bad_table |= akz_lt_start_bad(obs_start, n_landmarks, n_landmarks, n_obs);
    uint32_t rows = 0, observations = 0, empty = 0;
    for (uint32_t r = 0; r < n_landmarks; ++r) {
        uint32_t s, e;
        if (!akz_rp_row_range(obs_start, r, n_obs, &s, &e)) {
            bad_table = 1;
            continue;
        }
        for (uint32_t i = s; i < e; ++i) {
            const int k = akz_rp_observation(map, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], n_blocks, cap);
            if (k < 0) bad_index = 1;
            else kept[r] += (uint32_t)k;
        }
        rows += kept[r] != 0u;
        observations += kept[r];
        empty += s == e;
    }

    /* k_rp_scan_sums */
    const uint32_t verdict = akz_rp_verdict(bad_table, bad_map, bad_index, rows, observations, lm_room, obs_room);
    const int counted = akz_rp_counted(verdict), ok = verdict == AKZ_RP_OK;
    const uint32_t old_obs = counted ? obs_start[n_landmarks] - obs_start[0] : 0u;
    counts_out[AKZ_RP_C_ROWS] = counted ? rows : 0u;
    counts_out[AKZ_RP_C_OBSERVATIONS] = counted ? observations : 0u;
    counts_out[AKZ_RP_C_EMPTY_DROPPED] = counted ? empty : 0u;
    counts_out[AKZ_RP_C_ROWS_DROPPED] = counted ? n_landmarks - rows - empty : 0u;
    counts_out[AKZ_RP_C_OBS_DROPPED] = counted ? old_obs - observations : 0u;
    *call_verdict = verdict;

    /* k_rp_rows */
    uint32_t key = 0, dst = 0;
    for (uint32_t r = 0; r < n_landmarks; ++r) {
        const uint32_t n = kept[r];
        const int live = ok && n != 0u;
        key_out[r] = live ? key : AKZ_RP_NONE;
        kept[r] = key;                                  /* the kept rows below r */
        if (live) {
            obs_start_out[key] = dst;
            obs_counts_out[key] = n;
            for (uint32_t i = obs_start[r]; i < obs_start[r + 1]; ++i) {
                const uint32_t m = akz_rp_map(map, obs[2 * (size_t)i]), feat = obs[2 * (size_t)i + 1];
                if (m == AKZ_RP_NONE) continue;
                obs_out[2 * (size_t)dst] = m;
                obs_out[2 * (size_t)dst + 1] = feat;
                ++dst;
                uint32_t* w = landmarks_out + (size_t)m * cap + feat;
                if (key < *w) *w = key;
            }
        }
        key += n != 0u;
    }
    kept[n_landmarks] = rows;

    /* k_rp_tail */
    for (uint32_t r = ok ? rows : 0u; r <= lm_room; ++r) {
        obs_start_out[r] = ok ? observations : 0u;
        if (r < lm_room) obs_counts_out[r] = 0u;
    }
    if (recon_start_out)
        for (uint32_t r = 0; r <= n_recons; ++r) recon_start_out[r] = ok ? kept[recon_start[r]] : 0u;
    free(kept);
    return 0;
}

/* rs_gather_blocks_device on host arrays.  -1: out of memory. */
int rp_gather(const unsigned char* src, unsigned char* dst, uint32_t row_bytes, uint32_t n_blocks, const uint32_t* map, uint32_t n_blocks_out,
              uint32_t* verdict)
{
    uint32_t* inv = (uint32_t*)malloc(((size_t)n_blocks_out + 1) * sizeof(uint32_t));
    if (!inv) return -1;
    const int bad = rp_map_bad(map, n_blocks, n_blocks_out, inv);
    if (bad < 0) {
        free(inv);
        return -1;
    }
    for (uint32_t t = 0; t < n_blocks_out; ++t) {
        if (bad || inv[t] == AKZ_RP_NONE) memset(dst + (size_t)t * row_bytes, 0, row_bytes);
        else memcpy(dst + (size_t)t * row_bytes, src + (size_t)inv[t] * row_bytes, row_bytes);
    }
    *verdict = bad ? AKZ_RP_BAD_MAP : AKZ_RP_OK;
    free(inv);
    return 0;
}

/* rs_repack_constraints_device on host arrays.  -1: out of memory. */
int rp_constraints(const uint32_t* views, const double* poses, const uint32_t* cverdict, uint32_t n, const uint32_t* map, uint32_t n_blocks,
                   uint32_t n_blocks_out, const uint32_t* start, uint32_t n_ranges, uint32_t* views_out, double* poses_out,
                   uint32_t* cverdict_out, uint32_t* count, uint32_t* start_out)
{
    uint32_t* prefix = (uint32_t*)malloc(((size_t)n + 1) * sizeof(uint32_t));
    if (!prefix) return -1;
    uint32_t at = 0;
    for (uint32_t c = 0; c < n; ++c) {
        prefix[c] = at;
        if (!akz_rp_constraint_kept(map, views + 3 * (size_t)c, n_blocks, n_blocks_out)) continue;
        for (int k = 0; k < 3; ++k) views_out[3 * (size_t)at + k] = akz_rp_map(map, views[3 * (size_t)c + k]);
        cverdict_out[at] = cverdict[c];
        memcpy(poses_out + 24 * (size_t)at, poses + 24 * (size_t)c, 24 * sizeof(double));
        ++at;
    }
    prefix[n] = at;
    *count = at;
    for (uint32_t i = at; i < n; ++i) {
        for (int k = 0; k < 3; ++k) views_out[3 * (size_t)i + k] = AKZ_RP_NONE;
        cverdict_out[i] = AKZ_RP_TVC_BAD_INDEX;
        for (int k = 0; k < 24; ++k) poses_out[24 * (size_t)i + k] = 0.0;
    }
    if (start)
        for (uint32_t r = 0; r <= n_ranges; ++r) start_out[r] = prefix[start[r] < n ? start[r] : n];
    free(prefix);
    return 0;
}

/* hm_place_remap_views_device on host arrays */
void rp_frames(uint32_t* recon, uint32_t* view, uint32_t n_stored, uint32_t which, const uint32_t* map, uint32_t n_blocks, uint32_t* flags)
{
    *flags = 0u;
    for (uint32_t i = 0; i < n_stored; ++i) {
        uint32_t v = 0u;
        const int k = akz_rp_frame(map, recon[i], view[i], which, n_blocks, &v);
        if (k == 1) view[i] = v;
        if (k == 2) recon[i] = AKZ_RP_NONE;
        if (k < 0) *flags = 1u;
    }
}

/* ---- the constants, for the ABI test ---- */
uint32_t rp_constant(int which)
{
    const uint32_t v[] = {AKZ_RP_OK, AKZ_RP_BAD_TABLE, AKZ_RP_BAD_INDEX, AKZ_RP_BAD_MAP, AKZ_RP_NO_ROOM, AKZ_RP_COUNTS, AKZ_RP_TVC_BAD_INDEX};
    return v[which];
}
