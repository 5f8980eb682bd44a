/* The CPU checker of the covisibility search: thin exported wrappers around include/akz_covisibility_math.h, the text
 * cv_amd/csrc/rs_covisibility.hip compiles for the device.  tests/covisibility_checker.py has tests/host_build.py build this
 * with the host compiler into a shared object and loads it with ctypes.  The loops around the header (the inverse map, a
 * target's counts, its bit rows, the scan over the slots) restate the kernels' one after another, serially; every key, the
 * candidate cut, the walk, the chain and the record are the header's. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/akz_covisibility_math.h"

static int cmp_u64(const void* a, const void* b)
{
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : x > y ? 1 : 0;
}

static unsigned popcount64(uint64_t x)
{
    unsigned n = 0;
    for (; x; x &= x - 1) ++n;
    return n;
}

/* rs_covisibility_candidates_device on host arrays; -> 0, or -1 when memory ran out */
int cv_candidates(const uint32_t* obs_start, const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t cap, uint32_t n_blocks,
                  const unsigned char* reason, const uint32_t* targets, uint32_t n_targets, const akz_cv_settings* st, uint32_t* views,
                  uint32_t* lm_start, uint32_t* lm, uint32_t* slot_count, uint32_t* verdict, uint32_t* stats)
{
    const uint32_t limit = st->limit, minc = akz_cv_minimum(st), wmax = (cap + 63u) / 64u;
    const size_t n_slots = (size_t)n_targets * limit;
    uint32_t* inv = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)n_blocks * cap + 1));
    unsigned char* lm_bad = (unsigned char*)calloc((size_t)n_landmarks + 1, 1);
    uint32_t* local = (uint32_t*)malloc(sizeof(uint32_t) * (n_slots + 1));
    uint32_t* tot = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)n_targets + 1));
    uint32_t* cnt = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)n_blocks + 1));
    uint32_t* feat = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)cap + 1));
    uint32_t* hist = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)cap + 2));
    uint64_t* rows = (uint64_t*)malloc(sizeof(uint64_t) * ((size_t)AKZ_CV_MAX_CANDIDATE_VIEWS * wmax + 1));
    uint64_t* keys = (uint64_t*)malloc(sizeof(uint64_t) * 8192);
    uint16_t* feat_of = (uint16_t*)malloc(sizeof(uint16_t) * ((size_t)cap + 1));
    int rc = -1;
    if (!inv || !lm_bad || !local || !tot || !cnt || !feat || !hist || !rows || !keys || !feat_of) goto done;
    rc = 0;
    /* k_cv_scatter */
    uint32_t flags = 0;
    for (size_t k = 0; k < (size_t)n_blocks * cap; ++k) inv[k] = AKZ_CV_NONE;
    for (uint32_t l = 0; l < n_landmarks; ++l) {
        const uint32_t s = obs_start[l], e = obs_start[l + 1];
        if (s > e || e > n_obs) {
            flags = 1;
            lm_bad[l] = 1;
            continue;
        }
        for (uint32_t i = s; i < e; ++i) {
            const uint32_t blk = obs[2 * (size_t)i], f = obs[2 * (size_t)i + 1];
            if (blk >= n_blocks || f >= cap) lm_bad[l] = 1;
            else if (l < inv[(size_t)blk * cap + f]) inv[(size_t)blk * cap + f] = l;
        }
    }
    memset(lm, 0, sizeof(uint32_t) * 3 * n_slots * st->maximum_landmarks);
    /* k_cv_targets */
    for (uint32_t t = 0; t < n_targets; ++t) {
        const uint32_t v = targets[t];
        const size_t slot0 = (size_t)t * limit;
        uint32_t* w = stats + (size_t)AKZ_CV_STATS * t;
        int bad = v >= n_blocks || flags != 0;
        uint32_t nF = 0;
        if (!bad) {
            for (uint32_t b = 0; b < n_blocks; ++b) cnt[b] = 0;
            for (uint32_t j = 0; j < cap; ++j) {
                const uint32_t l = inv[(size_t)v * cap + j];
                if (l == AKZ_CV_NONE) continue;
                if (lm_bad[l]) {
                    bad = 1;
                    continue;
                }
                if (reason[l] != AKZ_CV_TRI_OK) continue;
                feat[nF++] = l;
                for (uint32_t i = obs_start[l]; i < obs_start[l + 1]; ++i)
                    if (obs[2 * (size_t)i] != v && akz_cv_first_of_block(obs, obs_start[l], i)) ++cnt[obs[2 * (size_t)i]];
            }
        }
        if (bad) {
            for (uint32_t k = 0; k < limit; ++k) {
                views[3 * (slot0 + k)] = views[3 * (slot0 + k) + 1] = views[3 * (slot0 + k) + 2] = 0;
                slot_count[slot0 + k] = 0;
                local[slot0 + k] = 0;
            }
            for (int k = 0; k < AKZ_CV_STATS; ++k) w[k] = 0;
            verdict[t] = AKZ_CV_BAD_INDEX;
            tot[t] = 0;
            continue;
        }
        for (uint32_t c = 0; c <= nF; ++c) hist[c] = 0;
        for (uint32_t b = 0; b < n_blocks; ++b)
            if (cnt[b] >= minc) ++hist[cnt[b]];
        uint32_t thr, quota, cand[AKZ_CV_MAX_CANDIDATE_VIEWS], C = 0, eq_run = 0;
        const int capped = akz_cv_candidate_threshold(hist, nF, minc, &thr, &quota);
        for (uint32_t b = 0; b < n_blocks; ++b) {
            const uint32_t c = cnt[b];
            int keep = c > thr && c >= minc;
            if (capped && c == thr) keep = keep || eq_run++ < quota;
            keep = keep && C < AKZ_CV_MAX_CANDIDATE_VIEWS;
            cnt[b] = keep ? C : AKZ_CV_NONE;
            if (keep) cand[C++] = b;
        }
        const uint32_t W = (nF + 63u) / 64u;
        for (uint32_t k = 0; k < C; ++k)
            for (uint32_t x = 0; x < W; ++x) rows[(size_t)k * wmax + x] = 0;
        for (uint32_t p = 0; p < nF; ++p) {
            const uint32_t l = feat[p];
            for (uint32_t i = obs_start[l]; i < obs_start[l + 1]; ++i) {
                const uint32_t blk = obs[2 * (size_t)i];
                const uint32_t ci = blk != v ? cnt[blk] : AKZ_CV_NONE;
                if (ci != AKZ_CV_NONE) rows[(size_t)ci * wmax + (p >> 6)] |= (uint64_t)1 << (p & 63u);
            }
        }
        const uint32_t P = C * (C - (C ? 1u : 0u)) / 2u;
        uint32_t n_pairs = 0;
        for (uint32_t q = 0; q < P; ++q) {
            uint32_t ia, ib, count = 0;
            akz_cv_pair_from_index(q, C, &ia, &ib);
            for (uint32_t x = 0; x < W; ++x) count += popcount64(rows[(size_t)ia * wmax + x] & rows[(size_t)ib * wmax + x]);
            if (count >= minc) keys[n_pairs++] = akz_cv_pair_key(count, q);
        }
        qsort(keys, n_pairs, sizeof(uint64_t), cmp_u64);
        unsigned char visited[AKZ_CV_MAX_CANDIDATE_VIEWS + 1];
        uint32_t unique[(AKZ_CV_MAX_PAIRS + 31) / 32 + 1];
        w[AKZ_CV_S_ROBUST] = nF;
        w[AKZ_CV_S_CANDIDATES] = C;
        w[AKZ_CV_S_FLAGS] = capped ? AKZ_CV_F_CANDIDATES_CAPPED : 0;
        w[AKZ_CV_S_RECORDED] = 0;
        w[7] = 0;
        tot[t] = akz_cv_walk(keys, n_pairs, cand, C, v, st, visited, unique, views + 3 * slot0, slot_count + slot0, local + slot0, w);
        verdict[t] = AKZ_CV_OK;
    }
    /* k_cv_scan */
    uint32_t carry = 0;
    for (uint32_t t = 0; t < n_targets; ++t) {
        const uint32_t n = tot[t];
        tot[t] = carry;
        carry += n;
    }
    lm_start[n_slots] = carry;
    /* k_cv_lists */
    for (size_t slot = 0; slot < n_slots; ++slot) {
        const uint32_t t = (uint32_t)(slot / limit), start = tot[t] + local[slot], count = slot_count[slot];
        lm_start[slot] = start;
        if (count == 0) continue;
        const uint32_t v = targets[t];
        const uint32_t* x = views + 3 * slot;
        const int vi = x[0] == v ? 0 : x[1] == v ? 1 : 2, ai = vi == 0 ? 1 : 0, bi = vi == 2 ? 1 : 2;
        uint32_t run = 0;
        for (uint32_t j = 0; j < cap; ++j) {
            const uint32_t l = inv[(size_t)v * cap + j];
            uint32_t f;
            if (l == AKZ_CV_NONE || reason[l] != AKZ_CV_TRI_OK) continue;
            const uint32_t s = obs_start[l], e = obs_start[l + 1];
            if (!akz_cv_find_view(obs, s, e, x[ai], &f) || !akz_cv_find_view(obs, s, e, x[bi], &f)) continue;
            keys[run] = akz_cv_list_key(akz_cv_distinct_views(obs, s, e), st->seed, l, run);
            feat_of[run] = (uint16_t)j;
            ++run;
        }
        qsort(keys, run, sizeof(uint64_t), cmp_u64);
        uint32_t take = count < st->maximum_landmarks ? count : st->maximum_landmarks;
        take = take < run ? take : run;
        for (uint32_t k = 0; k < take; ++k) {
            const uint32_t j = feat_of[akz_cv_list_key_pos(keys[k])];
            const uint32_t l = inv[(size_t)v * cap + j], s = obs_start[l], e = obs_start[l + 1];
            uint32_t fa = 0, fb = 0;
            akz_cv_find_view(obs, s, e, x[ai], &fa);
            akz_cv_find_view(obs, s, e, x[bi], &fb);
            uint32_t* row = lm + 3 * ((size_t)start + k);
            row[vi] = j;
            row[ai] = fa;
            row[bi] = fb;
        }
    }
done:
    free(inv); free(lm_bad); free(local); free(tot); free(cnt); free(feat); free(hist); free(rows); free(keys); free(feat_of);
    return rc;
}

/* rs_covisibility_record_device on host arrays: verdict and stats are the candidates call's, updated in place */
void cv_record(const uint32_t* constraint_verdict, const uint32_t* targets, uint32_t n_targets, const uint32_t* graph_start, uint32_t n_graphs,
               const akz_cv_settings* st, uint32_t* recorded, uint32_t* verdict, uint32_t* stats)
{
    for (uint32_t t = 0; t < n_targets; ++t) {
        const size_t slot0 = (size_t)t * st->limit;
        uint32_t n = 0;
        int out = (int)verdict[t];
        if (out == AKZ_CV_OK || out == AKZ_CV_FEW_CONSTRAINTS || out == AKZ_CV_NO_GRAPH) {
            const uint32_t views = akz_cv_graph_views(graph_start, n_graphs, targets[t]);
            out = views == AKZ_CV_NONE ? AKZ_CV_NO_GRAPH : akz_cv_record(constraint_verdict + slot0, st, views, recorded + slot0, &n);
        }
        if (out != AKZ_CV_OK && out != AKZ_CV_FEW_CONSTRAINTS)
            for (uint32_t k = 0; k < st->limit; ++k)
                recorded[slot0 + k] = constraint_verdict[slot0 + k] ? constraint_verdict[slot0 + k] : AKZ_CV_NOT_RECORDED;
        verdict[t] = (uint32_t)out;
        stats[(size_t)AKZ_CV_STATS * t + AKZ_CV_S_RECORDED] = n;
    }
}

/* rs_pose_graph_rows_device on host arrays: count, scan, ordered fill; row_edges has room for 6 n; -> the flag word */
uint32_t cv_rows(const uint32_t* views, uint32_t n, uint32_t n_views, uint32_t* row_start, uint32_t* row_edges)
{
    uint32_t flag = 0;
    uint32_t* cursor = (uint32_t*)calloc((size_t)n_views + 1, sizeof(uint32_t));
    if (!cursor) return 0xFFFFFFFFu;
    for (size_t k = 0; k < 6 * (size_t)n; ++k) row_edges[k] = 0;
    for (uint32_t c = 0; c < n; ++c) {
        const uint32_t* x = views + 3 * (size_t)c;
        if (x[0] >= n_views || x[1] >= n_views || x[2] >= n_views) flag = 1;
        else
            for (uint32_t s = 0; s < 6; ++s) ++cursor[x[AKZ_CV_SLOT_TARGET(s)]];
    }
    uint32_t carry = 0;
    for (uint32_t v = 0; v < n_views; ++v) {
        const uint32_t k = cursor[v];
        row_start[v] = cursor[v] = carry;
        carry += k;
    }
    row_start[n_views] = carry;
    for (uint32_t c = 0; c < n; ++c) {                      /* constraint ascending, slot ascending: every row ascends */
        const uint32_t* x = views + 3 * (size_t)c;
        if (x[0] >= n_views || x[1] >= n_views || x[2] >= n_views) continue;
        for (uint32_t s = 0; s < 6; ++s) row_edges[cursor[x[AKZ_CV_SLOT_TARGET(s)]]++] = 6 * c + s;
    }
    free(cursor);
    return flag;
}

/* ---- the pieces, for the rule tests ---- */
uint32_t cv_mix(uint32_t seed, uint32_t landmark) { return akz_cv_mix(seed, landmark); }
uint64_t cv_list_key(uint32_t n, uint32_t seed, uint32_t landmark, uint32_t pos) { return akz_cv_list_key(n, seed, landmark, pos); }
void cv_pair_from_index(uint32_t q, uint32_t n, uint32_t* ab) { akz_cv_pair_from_index(q, n, ab, ab + 1); }
int cv_record_one(const uint32_t* verdict, const akz_cv_settings* st, uint32_t graph_views, uint32_t* recorded, uint32_t* n)
{
    return akz_cv_record(verdict, st, graph_views, recorded, n);
}
