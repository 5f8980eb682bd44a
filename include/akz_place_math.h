/* akz_place_math.h — cv-sfm's choice of the frames a frame is compared with: the window of recent frames of its feed, the
 * nearest stored hashes, the three filters, the split by reconstruction and the order of the reconstructions.  All of it is
 * integers.  Written once for gcc (the CPU checker, tests/cpp/place_host.c) and hipcc (the gfx950 kernels of
 * cv_amd/csrc/hm_place.hip): parity is "host build == HIP" in every byte of every output.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlamData::find_visually_similar_and_recent_frames   cv-sfm/src/lib.rs:597-668
 *   try_localize: the reconstructions by views found     cv-sfm/src/lib.rs:853-855
 *   the defaults                                          cv-sfm/src/settings.rs:437-451
 *
 * Departures:
 *   - the search is exact, ascending (distance, row) over all bits of the hash, where the reference asks an approximate index
 *     (HggLite::knn_values): the statement hm_hash_knn documents;
 *   - a query sees the rows below its `visible` only: that is the reference's sequence (add_frame inserts, then asks);
 *   - the reference indexes the window by the position in the feed's own list; here that position is the table's `pos`, and a
 *     second visible frame on one slot of the window (the query's own slot included) is the verdict AKZ_PL_BAD_TABLE;
 *   - reconstructions with equally many views found: ascending reconstruction key (the reference: a HashMap's order and an
 *     unstable sort).
 */
#ifndef AKZ_PLACE_MATH_H
#define AKZ_PLACE_MATH_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define AKZ_PL_FN __host__ __device__ static inline
#else
#define AKZ_PL_FN static inline
#endif

/* the verdict on a query (HM_PL_* of include/akz.h) */
enum {
    AKZ_PL_OK = 0,
    AKZ_PL_BAD_INDEX = 1,       /* query >= n_stored, visible > n_stored or query >= visible: nothing is read through either */
    AKZ_PL_BAD_TABLE = 2        /* two visible frames on one slot of the query's window */
};
/* words of a query's row of d_counts */
enum { AKZ_PL_C_RECENT = 0, AKZ_PL_C_SIMILAR = 1, AKZ_PL_C_SEARCHED = 2, AKZ_PL_C_GROUPS = 3, AKZ_PL_C_FREE = 4, AKZ_PL_COUNTS = 5 };
/* the limits */
enum { AKZ_PL_MAX_HASH_BYTES = 4096, AKZ_PL_MAX_SEARCH = 2048, AKZ_PL_MAX_RECENT = 256 };
#define AKZ_PL_NONE 0xFFFFFFFFu

/* ---- sizes ---- */
/* slots of the window: the positions pos[q] - (num_recent - 1) .. pos[q] + (num_recent - 1), the query's own in the middle */
AKZ_PL_FN uint32_t akz_pl_window_slots(uint32_t num_recent) { return num_recent ? 2u * num_recent - 1u : 0u; }
/* the longest chain: every slot of the window but the query's own, and the similar frames */
AKZ_PL_FN uint32_t akz_pl_room(uint32_t num_similar, uint32_t num_recent)
{
    return (num_recent ? 2u * num_recent - 2u : 0u) + num_similar;
}
/* bins of the histogram of distances: 0 .. 8 * hash_bytes */
AKZ_PL_FN uint32_t akz_pl_bins(uint32_t hash_bytes) { return 8u * hash_bytes + 1u; }
/* the hashes a query's search returns */
AKZ_PL_FN uint32_t akz_pl_searched(uint32_t search_num, uint32_t visible) { return search_num < visible ? search_num : visible; }

/* ---- the query (the refusals of a query alone) ---- */
AKZ_PL_FN uint32_t akz_pl_query_verdict(uint32_t query, uint32_t visible, uint32_t n_stored)
{
    return (query >= n_stored || visible > n_stored || query >= visible) ? (uint32_t)AKZ_PL_BAD_INDEX : (uint32_t)AKZ_PL_OK;
}

/* ---- the search order ---- */
/* ascending keys are ascending (distance, row) */
AKZ_PL_FN unsigned long long akz_pl_key(uint32_t distance, uint32_t row) { return ((unsigned long long)distance << 32) | row; }
AKZ_PL_FN uint32_t akz_pl_key_row(unsigned long long key) { return (uint32_t)key; }
AKZ_PL_FN uint32_t akz_pl_key_distance(unsigned long long key) { return (uint32_t)(key >> 32); }

/* ---- the window (lib.rs:611-621) ---- */
/* |a - b| of two positions */
AKZ_PL_FN uint32_t akz_pl_abs_difference(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
/* Frame r (another row than the query's) against the query's window: 1 and its slot — ascending slots are ascending positions,
 * slot num_recent - 1 is the query's own position — or 0.  A frame on the query's own slot is a second frame of one (feed, pos). */
AKZ_PL_FN int akz_pl_window_slot(uint32_t feed_r, uint32_t pos_r, uint32_t feed_q, uint32_t pos_q, uint32_t num_recent, uint32_t* slot)
{
    if (feed_r != feed_q) return 0;
    const uint32_t ad = akz_pl_abs_difference(pos_r, pos_q);
    if (!(ad < num_recent)) return 0;
    *slot = pos_r >= pos_q ? num_recent - 1u + ad : num_recent - 1u - ad;
    return 1;
}
/* frames counted on a slot -> is the table broken there?  (the query's own slot holds the query already) */
AKZ_PL_FN int akz_pl_slot_bad(uint32_t slot, uint32_t count, uint32_t num_recent) { return count > (slot == num_recent - 1u ? 0u : 1u); }

/* ---- the three filters of the similar frames (lib.rs:626-636) ---- */
/* 1: a searched row stays.  It is dropped as the query itself, as a frame of the recent list — every visible frame of the query's
 * feed with |pos difference| < num_recent is in it, and every searched row is visible — or as too close in the feed. */
AKZ_PL_FN int akz_pl_similar_keeps(uint32_t row, uint32_t feed_r, uint32_t pos_r, uint32_t query, uint32_t feed_q, uint32_t pos_q,
                                   uint32_t num_recent, uint32_t recent_threshold)
{
    if (row == query) return 0;
    if (feed_r != feed_q) return 1;
    const uint32_t ad = akz_pl_abs_difference(pos_q, pos_r);
    return !(ad < num_recent) && !(ad < recent_threshold);
}

/* ---- the selection from a histogram ---- */
/* The bins [b0, b1) of a histogram of distances, `before` rows counted in the bins below b0, `wanted` >= 1 rows asked for in
 * ascending (distance, row) order: 1 when the wanted-th row falls into these bins — then every row below distance *threshold is
 * taken, and the first *quota >= 1 rows at it in row order — else 0, and *before_out = the rows counted below b1. */
AKZ_PL_FN int akz_pl_threshold_run(const uint32_t* hist, uint32_t b0, uint32_t b1, uint32_t before, uint32_t wanted, uint32_t* threshold,
                                   uint32_t* quota, uint32_t* before_out)
{
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t c = hist[b];
        if (wanted - before <= c) {
            *threshold = b;
            *quota = wanted - before;
            return 1;
        }
        before += c;
    }
    *before_out = before;
    return 0;
}
/* is a row at `distance` taken, given how many rows at the threshold lie before it in row order? */
AKZ_PL_FN int akz_pl_takes(uint32_t distance, uint32_t threshold, uint32_t rank_at_threshold, uint32_t quota)
{
    return distance < threshold || (distance == threshold && rank_at_threshold < quota);
}

/* ---- the groups (lib.rs:643-652, 853-855) ---- */
/* entries of the chain with a view, ascending: by reconstruction, then in chain order */
AKZ_PL_FN unsigned long long akz_pl_member_key(uint32_t recon, uint32_t chain_position) { return ((unsigned long long)recon << 32) | chain_position; }
/* groups, ascending: more views found first, equal counts by ascending reconstruction key */
AKZ_PL_FN unsigned long long akz_pl_group_key(uint32_t views_found, uint32_t recon)
{
    return ((unsigned long long)(0xFFFFFFFFu - views_found) << 32) | recon;
}

/* ---- the host's execution of one query (the kernels' steps of hm_place.hip one after another) ---- */
AKZ_PL_FN uint32_t akz_pl_hamming(const uint8_t* a, const uint8_t* b, uint32_t hash_bytes)
{
    uint32_t d = 0;
    for (uint32_t k = 0; k < hash_bytes; ++k) {
        uint32_t x = (uint32_t)(a[k] ^ b[k]);
        for (; x; x &= x - 1u) ++d;
    }
    return d;
}
AKZ_PL_FN void akz_pl_sort_keys(unsigned long long* key, uint32_t n)
{
    for (uint32_t i = 1; i < n; ++i) {
        const unsigned long long k = key[i];
        uint32_t j = i;
        for (; j > 0 && key[j - 1] > k; --j) key[j] = key[j - 1];
        key[j] = k;
    }
}
/* One query of hm_find_frames_batch_device on host arrays.  The outputs are the query's rows (found, views_out, group_recon, free:
 * room words; group_start: room + 1; search: search_num {row, distance} pairs or null; counts: AKZ_PL_COUNTS; verdict: 1); what
 * the device does not write is not written.  hist: akz_pl_bins(hash_bytes) words; keys: max(search_num, room) + room keys. */
AKZ_PL_FN void akz_pl_find_one(const uint8_t* hashes, const uint32_t* feed, const uint32_t* pos, const uint32_t* recon, const uint32_t* view,
                               uint32_t n_stored, uint32_t hash_bytes, uint32_t query, uint32_t visible, uint32_t num_similar, uint32_t num_recent,
                               uint32_t recent_threshold, uint32_t search_num, uint32_t* found, uint32_t* views_out, uint32_t* group_recon,
                               uint32_t* group_start, uint32_t* free_out, uint32_t* search, uint32_t* counts, uint32_t* verdict, uint32_t* hist,
                               unsigned long long* keys)
{
    for (int k = 0; k < AKZ_PL_COUNTS; ++k) counts[k] = 0u;
    *verdict = akz_pl_query_verdict(query, visible, n_stored);
    if (*verdict != AKZ_PL_OK) return;
    const uint32_t feed_q = feed[query], pos_q = pos[query];
    /* the window */
    const uint32_t slots = akz_pl_window_slots(num_recent);
    uint32_t n_recent = 0;
    for (uint32_t s = 0; s < slots; ++s) {
        uint32_t count = 0, row = AKZ_PL_NONE;
        for (uint32_t r = 0; r < visible; ++r) {
            uint32_t at;
            if (r != query && akz_pl_window_slot(feed[r], pos[r], feed_q, pos_q, num_recent, &at) && at == s) {
                ++count;
                row = r;
            }
        }
        if (akz_pl_slot_bad(s, count, num_recent)) {
            *verdict = AKZ_PL_BAD_TABLE;
            return;
        }
        if (count) keys[n_recent++] = row;                      /* (nothing of a refused query's rows is written) */
    }
    for (uint32_t e = 0; e < n_recent; ++e) found[e] = (uint32_t)keys[e];
    /* the search */
    const uint32_t wanted = akz_pl_searched(search_num, visible);
    uint32_t n_similar = 0;
    if (wanted && (num_similar || search)) {
        const uint32_t bins = akz_pl_bins(hash_bytes);
        for (uint32_t b = 0; b < bins; ++b) hist[b] = 0u;
        for (uint32_t r = 0; r < visible; ++r) ++hist[akz_pl_hamming(hashes + (size_t)query * hash_bytes, hashes + (size_t)r * hash_bytes, hash_bytes)];
        uint32_t threshold = 0, quota = 0, before = 0;
        (void)akz_pl_threshold_run(hist, 0u, bins, 0u, wanted, &threshold, &quota, &before);
        uint32_t n = 0, at = 0;
        for (uint32_t r = 0; r < visible; ++r) {
            const uint32_t d = akz_pl_hamming(hashes + (size_t)query * hash_bytes, hashes + (size_t)r * hash_bytes, hash_bytes);
            if (akz_pl_takes(d, threshold, at, quota)) keys[n++] = akz_pl_key(d, r);
            at += d == threshold;
        }
        akz_pl_sort_keys(keys, n);
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t r = akz_pl_key_row(keys[j]);
            if (search) {
                search[2 * (size_t)j] = r;
                search[2 * (size_t)j + 1] = akz_pl_key_distance(keys[j]);
            }
            if (n_similar < num_similar && akz_pl_similar_keeps(r, feed[r], pos[r], query, feed_q, pos_q, num_recent, recent_threshold))
                found[n_recent + n_similar++] = r;
        }
    }
    /* the chain by reconstruction */
    const uint32_t n_chain = n_recent + n_similar;
    uint32_t n_free = 0, n_members = 0, n_groups = 0;
    unsigned long long* gkeys = keys + n_chain;
    for (uint32_t e = 0; e < n_chain; ++e) {
        if (recon[found[e]] == AKZ_PL_NONE) free_out[n_free++] = found[e];
        else keys[n_members++] = akz_pl_member_key(recon[found[e]], e);
    }
    akz_pl_sort_keys(keys, n_members);
    for (uint32_t m = 0; m < n_members;) {
        uint32_t e = m;
        while (e < n_members && (uint32_t)(keys[e] >> 32) == (uint32_t)(keys[m] >> 32)) ++e;
        gkeys[n_groups++] = akz_pl_group_key(e - m, (uint32_t)(keys[m] >> 32));
        m = e;
    }
    akz_pl_sort_keys(gkeys, n_groups);
    uint32_t out = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t key = (uint32_t)gkeys[g];
        group_recon[g] = key;
        group_start[g] = out;
        for (uint32_t m = 0; m < n_members; ++m)
            if ((uint32_t)(keys[m] >> 32) == key) views_out[out++] = view[found[(uint32_t)keys[m]]];
    }
    group_start[n_groups] = out;
    counts[AKZ_PL_C_RECENT] = n_recent;
    counts[AKZ_PL_C_SIMILAR] = n_similar;
    counts[AKZ_PL_C_SEARCHED] = wanted;
    counts[AKZ_PL_C_GROUPS] = n_groups;
    counts[AKZ_PL_C_FREE] = n_free;
}

#endif /* AKZ_PLACE_MATH_H */
