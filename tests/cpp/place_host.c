/* The CPU checker of the place-recognition kernels: the host's execution of one query is in include/akz_place_math.h itself (the
 * kernels' steps of cv_amd/csrc/hm_place.hip one after another, around the decisions the kernels compile for the device); this
 * file runs it over a batch.  tests/test_place_statement.py has tests/host_build.py build it with the host compiler into a shared
 * object and loads it with ctypes.  Every output buffer is produced whole: what the device call does not write is not written
 * here either, so that both sides can start from one fill.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_place_math.h"

/* hm_find_frames_batch_device on host arrays; -1: no memory */
int pl_find(const uint8_t* hashes, const uint32_t* feed, const uint32_t* pos, const uint32_t* recon, const uint32_t* view, uint32_t n_stored,
            uint32_t hash_bytes, const uint32_t* query, const uint32_t* visible, uint32_t nq, uint32_t num_similar, uint32_t num_recent,
            uint32_t recent_threshold, uint32_t search_num, uint32_t room, uint32_t* found, uint32_t* views_out, uint32_t* group_recon,
            uint32_t* group_start, uint32_t* free_out, uint32_t* search, uint32_t* counts, uint32_t* verdict)
{
    const uint32_t need = akz_pl_room(num_similar, num_recent);
    uint32_t* hist = (uint32_t*)malloc(sizeof(uint32_t) * akz_pl_bins(hash_bytes));
    unsigned long long* keys = (unsigned long long*)malloc(sizeof(unsigned long long) * ((size_t)(search_num > need ? search_num : need) + need + 1));
    if (!hist || !keys) {
        free(hist);
        free(keys);
        return -1;
    }
    for (uint32_t q = 0; q < nq; ++q)
        akz_pl_find_one(hashes, feed, pos, recon, view, n_stored, hash_bytes, query[q], visible ? visible[q] : n_stored, num_similar, num_recent,
                        recent_threshold, search_num, found + (size_t)q * room, views_out + (size_t)q * room, group_recon + (size_t)q * room,
                        group_start + (size_t)q * (room + 1), free_out + (size_t)q * room, search ? search + 2 * (size_t)q * search_num : 0,
                        counts + (size_t)q * AKZ_PL_COUNTS, verdict + q, hist, keys);
    free(hist);
    free(keys);
    return 0;
}

/* ---- the pieces, for the rule tests ---- */
uint32_t pl_room(uint32_t num_similar, uint32_t num_recent) { return akz_pl_room(num_similar, num_recent); }
int pl_window_slot(uint32_t feed_r, uint32_t pos_r, uint32_t feed_q, uint32_t pos_q, uint32_t num_recent, uint32_t* slot)
{
    return akz_pl_window_slot(feed_r, pos_r, feed_q, pos_q, num_recent, slot);
}
int pl_similar_keeps(uint32_t row, uint32_t feed_r, uint32_t pos_r, uint32_t query, uint32_t feed_q, uint32_t pos_q, uint32_t num_recent,
                     uint32_t recent_threshold)
{
    return akz_pl_similar_keeps(row, feed_r, pos_r, query, feed_q, pos_q, num_recent, recent_threshold);
}
int pl_threshold(const uint32_t* hist, uint32_t bins, uint32_t wanted, uint32_t* threshold, uint32_t* quota)
{
    uint32_t before = 0;
    return akz_pl_threshold_run(hist, 0u, bins, 0u, wanted, threshold, quota, &before);
}
unsigned long long pl_key(uint32_t distance, uint32_t row) { return akz_pl_key(distance, row); }
unsigned long long pl_group_key(uint32_t views_found, uint32_t recon) { return akz_pl_group_key(views_found, recon); }
