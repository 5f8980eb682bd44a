/* The CPU checker of the landmark-table kernels: the loops of cv_amd/csrc/rs_landmark_table.hip restated one after another
 * around include/akz_landmark_table_math.h, the text the kernels compile for the device.  tests/landmark_table_checker.py has
 * tests/host_build.py build this with the host compiler into a shared object and loads it with ctypes.  Every output buffer is
 * produced whole: what the device call does not write is not written here either, so that both sides can start from one fill. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/akz_landmark_table_math.h"

/* rs_landmarks_sharing_view_device on host arrays */
void lt_sharing(const uint32_t* obs_start, const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, const uint32_t* best,
                const uint32_t* decision, uint32_t cap, uint32_t n_frames, unsigned char* merge_ok)
{
    const uint32_t fill = akz_lt_fill(obs_start, n_landmarks, n_obs);
    for (size_t at = 0; at < (size_t)n_frames * cap; ++at) {
        uint32_t sa, ea, sb, eb;
        merge_ok[at] = akz_lt_candidate(obs_start, n_landmarks, fill, decision[at], best + 6 * at, &sa, &ea, &sb, &eb) &&
                       !akz_lt_lists_share(obs, sa, ea, sb, eb);
    }
}

typedef struct lt_out {
    uint32_t* obs_out;
    uint32_t* landmarks_out;
    uint32_t cap, n_blocks;
} lt_out;
static void lt_put(const lt_out* o, uint32_t at, uint32_t blk, uint32_t feat, uint32_t key)
{
    o->obs_out[2 * (size_t)at] = blk;
    o->obs_out[2 * (size_t)at + 1] = feat;
    if (blk < o->n_blocks && feat < o->cap) {
        uint32_t* w = o->landmarks_out + (size_t)blk * o->cap + feat;
        if (key < *w) *w = key;
    }
}

/* rs_add_views_device on host arrays (the refusals of the entry point are not restated: the caller keeps its rooms).  -1: out
 * of memory. */
int lt_add_views(const uint32_t* obs_start, const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t n_world, const uint32_t* split,
                 const uint32_t* split_count, uint32_t split_room, uint32_t cap, uint32_t n_blocks, const uint32_t* ik, uint32_t n_frames,
                 const uint32_t* counts, const uint32_t* matches, const uint32_t* nmatches, const unsigned char* final_mask,
                 const uint32_t* sv_verdict, const double* pose_out, const uint32_t* best, const uint32_t* skip, uint32_t obs_room,
                 uint32_t lm_room, double* poses, uint32_t* obs_start_out, uint32_t* obs_out, uint32_t* counts_out, uint32_t* landmarks_out,
                 uint32_t* obs_counts_out, uint32_t* frame_verdict, uint32_t* stats, uint32_t* call_verdict)
{
    const size_t nl = (size_t)n_landmarks + 1, nf = (size_t)n_frames + 1;
    uint32_t* refs = (uint32_t*)calloc(nl, sizeof(uint32_t));
    uint32_t* adds = (uint32_t*)calloc(nl, sizeof(uint32_t));
    uint32_t* cursor = (uint32_t*)calloc(nl, sizeof(uint32_t));
    uint32_t* merged_into = (uint32_t*)malloc(nl * sizeof(uint32_t));
    uint32_t* merged_from = (uint32_t*)malloc(nl * sizeof(uint32_t));
    uint32_t* block_slot = (uint32_t*)malloc((size_t)n_blocks * sizeof(uint32_t));
    uint32_t* accepted = (uint32_t*)calloc(nf, sizeof(uint32_t));
    uint32_t* new_rows = (uint32_t*)calloc(nf, sizeof(uint32_t));
    uint32_t* feat = (uint32_t*)malloc(((size_t)n_frames * cap + 1) * sizeof(uint32_t));
    int status = -1;
    (void)obs_room;
    if (!refs || !adds || !cursor || !merged_into || !merged_from || !block_slot || !accepted || !new_rows || !feat) goto done;
    status = 0;
    memset(merged_into, 0xFF, nl * sizeof(uint32_t));
    memset(merged_from, 0xFF, nl * sizeof(uint32_t));
    memset(block_slot, 0xFF, (size_t)n_blocks * sizeof(uint32_t));
    memset(feat, 0xFF, ((size_t)n_frames * cap + 1) * sizeof(uint32_t));
    memset(landmarks_out, 0xFF, (size_t)n_blocks * cap * sizeof(uint32_t));
    const lt_out out = {obs_out, landmarks_out, cap, n_blocks};

    /* k_lt_check_table */
    int bad_table = 0;
    for (uint32_t l = 0; l <= n_landmarks; ++l) bad_table |= akz_lt_start_bad(obs_start, l, n_landmarks, n_obs);

    /* k_lt_validate */
    for (uint32_t f = 0; f < n_frames; ++f) {
        const uint32_t blk = ik[f], count = counts[blk], nm = nmatches[f];
        const int off = bad_table || sv_verdict[f] != (uint32_t)AKZ_LT_SV_OK || (skip && skip[f] != 0u);
        int bad = count > cap || nm > cap;
        uint32_t n_final = 0;
        block_slot[blk] = f;
        if (!off && !bad) {
            for (uint32_t i = 0; i < nm; ++i) {
                const size_t at = (size_t)f * cap + i;
                uint32_t la, lb;
                if (!final_mask[at]) continue;
                const uint32_t feature = matches[2 * at];
                if (akz_lt_match(feature, matches[2 * at + 1], count, f, cap, n_world, n_landmarks, best, &la, &lb) == AKZ_LT_MATCH_BAD) bad = 1;
                else if (feat[(size_t)f * cap + feature] != AKZ_LT_NONE) bad = 1;
                else {
                    feat[(size_t)f * cap + feature] = i;
                    ++n_final;
                }
            }
        }
        accepted[f] = !off && !bad;
        new_rows[f] = accepted[f] ? count - n_final : 0u;
        frame_verdict[f] = off ? AKZ_AV_NOT_ACCEPTED : accepted[f] ? AKZ_AV_OK : AKZ_AV_BAD_INDEX;
        uint32_t* st = stats + (size_t)AKZ_AV_STATS * f;
        st[AKZ_AV_S_OBSERVATIONS] = accepted[f] ? n_final : 0u;
        st[AKZ_AV_S_MERGED] = 0u;
        st[AKZ_AV_S_DEMOTED] = 0u;
        st[AKZ_AV_S_NEW_LANDMARKS] = new_rows[f];
        if (accepted[f])
            for (int k = 0; k < 12; ++k) poses[(size_t)12 * blk + k] = pose_out[(size_t)12 * f + k];
    }

    /* k_lt_refs, then k_lt_merges on the complete counts */
    uint32_t n_merged = 0, n_demoted = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t f = 0; f < n_frames; ++f) {
            if (!accepted[f]) continue;
            for (uint32_t i = 0; i < nmatches[f]; ++i) {
                const size_t at = (size_t)f * cap + i;
                uint32_t la, lb;
                if (!final_mask[at]) continue;
                const int kind = akz_lt_match(matches[2 * at], matches[2 * at + 1], counts[ik[f]], f, cap, n_world, n_landmarks, best, &la, &lb);
                if (pass == 0) {
                    ++refs[la];
                    if (kind == AKZ_LT_MATCH_MERGED) ++refs[lb];
                    continue;
                }
                ++adds[la];
                if (kind != AKZ_LT_MATCH_MERGED) continue;
                if (akz_lt_merge_applied(refs[la], refs[lb])) {
                    merged_from[la] = lb;
                    merged_into[lb] = la;
                    ++stats[(size_t)AKZ_AV_STATS * f + AKZ_AV_S_MERGED];
                    ++n_merged;
                } else {
                    ++stats[(size_t)AKZ_AV_STATS * f + AKZ_AV_S_DEMOTED];
                    ++n_demoted;
                }
            }
        }

    /* k_lt_tile_sums .. k_lt_rows: the rows of the input table */
    uint32_t total_old = 0;
    for (uint32_t r = 0; r < n_landmarks; ++r) {
        uint32_t len = 0;
        const uint32_t m = merged_from[r];
        if (!bad_table) {
            const uint32_t merged = m != AKZ_LT_NONE ? obs_start[m + 1] - obs_start[m] : 0u;
            len = akz_lt_row_length(obs_start[r + 1] - obs_start[r], merged, adds[r], merged_into[r] != AKZ_LT_NONE);
        }
        obs_counts_out[r] = len;
        obs_start_out[r] = total_old;
        if (len) {
            uint32_t dst = total_old;
            for (uint32_t i = obs_start[r]; i < obs_start[r + 1]; ++i) lt_put(&out, dst++, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], r);
            if (m != AKZ_LT_NONE)
                for (uint32_t i = obs_start[m]; i < obs_start[m + 1]; ++i) lt_put(&out, dst++, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], r);
        }
        total_old += len;
    }

    /* k_lt_scan_sums: the totals */
    uint32_t rows = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
        const uint32_t v = new_rows[f];
        new_rows[f] = rows;
        rows += v;
    }
    uint32_t n_split = 0;
    if (!bad_table && split) n_split = *split_count < split_room ? *split_count : split_room;
    const uint32_t rows_filled = bad_table ? 0u : n_landmarks + n_split + rows;
    counts_out[AKZ_AV_C_ROWS] = rows_filled;
    counts_out[AKZ_AV_C_OBSERVATIONS] = total_old + n_split + rows;
    counts_out[AKZ_AV_C_MERGED] = n_merged;
    counts_out[AKZ_AV_C_DEMOTED] = n_demoted;
    *call_verdict = bad_table ? AKZ_AV_BAD_TABLE : AKZ_AV_OK;

    /* k_lt_tail */
    for (uint32_t r = n_landmarks; r <= lm_room; ++r) {
        const uint32_t at = bad_table ? 0u : akz_lt_tail_start(total_old, rows_filled, n_landmarks, r);
        obs_start_out[r] = at;
        if (r < lm_room) obs_counts_out[r] = r < rows_filled ? 1u : 0u;
        if (!bad_table && r - n_landmarks < n_split) lt_put(&out, at, split[2 * (size_t)(r - n_landmarks)], split[2 * (size_t)(r - n_landmarks) + 1], r);
    }

    /* k_lt_place, k_lt_new_rows */
    for (uint32_t f = 0; f < n_frames; ++f) {
        if (!accepted[f]) continue;
        const uint32_t blk = ik[f], count = counts[blk];
        for (uint32_t i = 0; i < nmatches[f]; ++i) {
            const size_t at = (size_t)f * cap + i;
            uint32_t la, lb;
            if (!final_mask[at]) continue;
            akz_lt_match(matches[2 * at], matches[2 * at + 1], count, f, cap, n_world, n_landmarks, best, &la, &lb);
            lt_put(&out, obs_start_out[la + 1] - adds[la] + cursor[la]++, blk, matches[2 * at], la);
        }
        uint32_t row = n_landmarks + n_split + new_rows[f];
        for (uint32_t j = 0; j < count; ++j)
            if (feat[(size_t)f * cap + j] == AKZ_LT_NONE) {
                lt_put(&out, akz_lt_tail_start(total_old, rows_filled, n_landmarks, row), blk, j, row);
                ++row;
            }
    }

    /* k_lt_fixup */
    for (uint32_t r = 0; r < n_landmarks; ++r) {
        const uint32_t n = adds[r];
        if (n < 2u) continue;
        uint32_t* tail = obs_out + 2 * (size_t)(obs_start_out[r + 1] - n);
        for (uint32_t i = 1; i < n; ++i) {
            const uint32_t ob = tail[2 * i], of = tail[2 * i + 1], slot = block_slot[ob];
            uint32_t k = i;
            while (k > 0u && akz_lt_tail_less(slot, of, block_slot[tail[2 * (k - 1u)]], tail[2 * (k - 1u) + 1])) {
                tail[2 * k] = tail[2 * (k - 1u)];
                tail[2 * k + 1] = tail[2 * (k - 1u) + 1];
                --k;
            }
            tail[2 * k] = ob;
            tail[2 * k + 1] = of;
        }
    }
done:
    free(refs); free(adds); free(cursor); free(merged_into); free(merged_from); free(block_slot); free(accepted); free(new_rows); free(feat);
    return status;
}

/* ---- the pieces, for the rule tests ---- */
int lt_merge_applied(uint32_t refs_a, uint32_t refs_b) { return akz_lt_merge_applied(refs_a, refs_b); }
int lt_lists_share(const uint32_t* obs, uint32_t sa, uint32_t ea, uint32_t sb, uint32_t eb) { return akz_lt_lists_share(obs, sa, ea, sb, eb); }
