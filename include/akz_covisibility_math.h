/* akz_covisibility_math.h — the covisibility search that feeds cv-sfm's three-view constraints (VSlam::generate_view_constraints
 * up to its call of optimize_three_view), the verdict of record_view_constraints and the rows of flatten_constraints, as plain
 * integer logic: gcc (the CPU checker, tests/cpp/covisibility_host.c) and hipcc (the gfx950 kernels of
 * cv_amd/csrc/rs_covisibility.hip) compile the same text.  Parity is "host build == HIP" in every output word.  There is no
 * floating point here.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlam::view_covisibilities                          cv-sfm/src/lib.rs:2535-2556
 *   VSlam::generate_view_constraints                    cv-sfm/src/lib.rs:2438-2516
 *   VSlam::optimize_three_view, up to its matches       cv-sfm/src/lib.rs:1939-1990
 *   VSlam::record_view_constraints                      cv-sfm/src/lib.rs:2092-2109
 *   VSlam::flatten_constraints                          cv-sfm/src/lib.rs:2519-2532
 *   the five settings                                   cv-sfm/src/settings.rs:453-475
 *
 * Unpinned against the reference, which walks HashMaps and sorts unstably here; this header fixes ONE admissible
 * order:
 *   - candidate views ascending by block; their pairs (a, b), a < b, lexicographic in that order;
 *   - the sort of the triples by covisible count is stable: equal counts keep the lexicographic order (akz_cv_pair_key);
 *   - a triple's landmarks are taken in the target's feature order and sorted stably by observation count, descending
 *     (akz_cv_list_key); the reference shuffles them first "to avoid bias" (lib.rs:1968) with the host's RNG: here equal counts
 *     are ordered by position when shuffle_seed == 0 and by akz_cv_mix(shuffle_seed, landmark), then position, otherwise;
 *   - a list that names a view twice counts once for that view, in the covisibility counts and in the landmark's observation
 *     count alike (the reference's observations are a map), and the first entry gives the feature;
 *   - more than AKZ_CV_MAX_CANDIDATE_VIEWS candidates: the ones with the largest counts stay, ties to the lower block
 *     (akz_cv_candidate_threshold); the reference has no such bound.
 */
#ifndef AKZ_COVISIBILITY_MATH_H
#define AKZ_COVISIBILITY_MATH_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define AKZ_CV_FN __host__ __device__ static inline
#else
#define AKZ_CV_FN static inline
#endif

enum {
    AKZ_CV_MAX_CANDIDATE_VIEWS = 128,   /* candidate views of a target */
    AKZ_CV_MAX_PAIRS = 8128,            /* 128 * 127 / 2 */
    AKZ_CV_MAX_SLOTS = 256,             /* candidate_limit at the most */
    AKZ_CV_MAX_FEATURES = 8192,         /* cap_per_img at the most: a position in a target's list is 13 bits of a sort key */
    AKZ_CV_MAX_LANDMARKS = 256          /* optimization_maximum_landmarks at the most (RS_TVC_MAX_LANDMARKS) */
};
/* a target's verdict (RS_CV_* of include/akz.h) */
enum {
    AKZ_CV_OK = 0,
    AKZ_CV_FEW_CONSTRAINTS = 1,   /* record_view_constraints returned false (lib.rs:2098-2102) */
    AKZ_CV_BAD_INDEX = 2,         /* the target, one of its landmarks' observations or the start array is out of bounds */
    AKZ_CV_NO_GRAPH = 3           /* no range of d_graph_start holds the target */
};
enum { AKZ_CV_NOT_RECORDED = 16 };   /* d_recorded of an accepted constraint that was not recorded (above every RS_TVC_*) */
/* stats words (u32) of a target */
enum {
    AKZ_CV_S_ROBUST = 0,        /* features of the target whose landmark is robust */
    AKZ_CV_S_CANDIDATES = 1,    /* candidate views kept */
    AKZ_CV_S_PAIRS = 2,         /* triples at or above the covisibility minimum */
    AKZ_CV_S_UNIQUE = 3,        /* triples the unique walk took */
    AKZ_CV_S_EMITTED = 4,       /* slots filled */
    AKZ_CV_S_FLAGS = 5,         /* AKZ_CV_F_* */
    AKZ_CV_S_RECORDED = 6,      /* constraints recorded (written by the record stage; 0 before) */
    AKZ_CV_STATS = 8            /* word 7 is 0 */
};
enum {
    AKZ_CV_F_CANDIDATES_CAPPED = 1,   /* more than AKZ_CV_MAX_CANDIDATE_VIEWS candidate views: the largest counts were kept */
    AKZ_CV_F_LIMIT_REACHED = 2        /* the chain held further admissible triples beyond the limit */
};
#define AKZ_CV_NONE 0xFFFFFFFFu
enum { AKZ_CV_TRI_OK = 0 };   /* RS_TRI_OK: the reason byte of a robust landmark */

typedef struct akz_cv_settings {
    uint32_t covisibility_minimum;   /* optimization_robust_covisibility_minimum_landmarks */
    uint32_t maximum_constraints;    /* optimization_maximum_three_view_constraints */
    uint32_t minimum_new;            /* optimization_minimum_new_constraints */
    uint32_t minimum_landmarks;      /* optimization_minimum_landmarks */
    uint32_t maximum_landmarks;      /* optimization_maximum_landmarks */
    uint32_t limit;                  /* slots per target: candidate_limit, or maximum_constraints when that is 0 */
    uint32_t seed;                   /* shuffle_seed */
} akz_cv_settings;

/* a view with no landmark is no key of the reference's map: the minimum that counts is at least 1 */
AKZ_CV_FN uint32_t akz_cv_minimum(const akz_cv_settings* st) { return st->covisibility_minimum ? st->covisibility_minimum : 1u; }

/* THE MIX of (shuffle_seed, landmark index): the 32-bit finaliser of MurmurHash3 over seed ^ landmark * 0x9E3779B9 */
AKZ_CV_FN uint32_t akz_cv_mix(uint32_t seed, uint32_t landmark)
{
    uint32_t h = seed ^ (landmark * 0x9E3779B9u);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

/* The key of a landmark of a triple's list; ascending keys = observation count descending, then the mix (0 for seed 0), then
 * position `pos` (< AKZ_CV_MAX_FEATURES) in the target's feature order.  Counts above 2^19 - 1 compare equal. */
AKZ_CV_FN uint64_t akz_cv_list_key(uint32_t n_observations, uint32_t seed, uint32_t landmark, uint32_t pos)
{
    const uint32_t c = n_observations < 0x7FFFFu ? n_observations : 0x7FFFFu;
    const uint32_t m = seed ? akz_cv_mix(seed, landmark) : 0u;
    return (uint64_t)(0x7FFFFu - c) << 45 | (uint64_t)m << 13 | (uint64_t)(pos & 0x1FFFu);
}
AKZ_CV_FN uint32_t akz_cv_list_key_pos(uint64_t key) { return (uint32_t)(key & 0x1FFFu); }

/* The key of pair q with `count` covisible landmarks; ascending keys = count descending, then q ascending (stable) */
AKZ_CV_FN uint64_t akz_cv_pair_key(uint32_t count, uint32_t q) { return (uint64_t)(0xFFFFFFFFu - count) << 32 | q; }
AKZ_CV_FN uint32_t akz_cv_pair_key_count(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)(key >> 32); }
AKZ_CV_FN uint32_t akz_cv_pair_key_index(uint64_t key) { return (uint32_t)key; }

/* pairs (a, b), a < b < n, in lexicographic order: the index of (a, a + 1) */
AKZ_CV_FN uint32_t akz_cv_pair_offset(uint32_t a, uint32_t n) { return a * (2u * n - a - 1u) / 2u; }
AKZ_CV_FN void akz_cv_pair_from_index(uint32_t q, uint32_t n, uint32_t* a, uint32_t* b)
{
    uint32_t lo = 0u, hi = n - 2u;                    /* the largest a with offset(a) <= q; n >= 2 */
    for (int k = 0; k < 8 && lo < hi; ++k) {          /* n <= 128: 7 halvings */
        const uint32_t mid = (lo + hi + 1u) / 2u;
        if (akz_cv_pair_offset(mid, n) <= q) lo = mid;
        else hi = mid - 1u;
    }
    *a = lo;
    *b = q - akz_cv_pair_offset(lo, n) + lo + 1u;
}

/* Which candidate views stay: hist[c] = views with count c, minimum <= c <= top.  A view stays when its count is above
 * *threshold, or equal to it and it is among the first *quota such views in block order.  -> 1 when the cap cut some off. */
AKZ_CV_FN int akz_cv_candidate_threshold(const uint32_t* hist, uint32_t top, uint32_t minimum, uint32_t* threshold, uint32_t* quota)
{
    uint32_t acc = 0u;
    for (uint32_t c = top; c >= minimum && c != 0u; --c) {
        if (acc + hist[c] > (uint32_t)AKZ_CV_MAX_CANDIDATE_VIEWS) {
            *threshold = c;
            *quota = (uint32_t)AKZ_CV_MAX_CANDIDATE_VIEWS - acc;
            return 1;
        }
        acc += hist[c];
    }
    *threshold = minimum - 1u;
    *quota = 0u;
    return 0;
}

/* does list obs[s .. e) ({block, feature} rows) name `view`?  the FIRST entry's feature */
AKZ_CV_FN int akz_cv_find_view(const uint32_t* obs, uint32_t s, uint32_t e, uint32_t view, uint32_t* feature)
{
    for (uint32_t i = s; i < e; ++i)
        if (obs[2 * (size_t)i] == view) {
            *feature = obs[2 * (size_t)i + 1];
            return 1;
        }
    return 0;
}
/* is entry i of list obs[s .. e) the first of its block? */
AKZ_CV_FN int akz_cv_first_of_block(const uint32_t* obs, uint32_t s, uint32_t i)
{
    const uint32_t blk = obs[2 * (size_t)i];
    for (uint32_t k = s; k < i; ++k)
        if (obs[2 * (size_t)k] == blk) return 0;
    return 1;
}

/* observations.len() of the reference's map: the distinct blocks of list obs[s .. e) */
AKZ_CV_FN uint32_t akz_cv_distinct_views(const uint32_t* obs, uint32_t s, uint32_t e)
{
    uint32_t n = 0u;
    for (uint32_t i = s; i < e; ++i) n += akz_cv_first_of_block(obs, s, i) ? 1u : 0u;
    return n;
}

/* canonical_view_order([v, a, b]) for a < b, both != v: ascending */
AKZ_CV_FN void akz_cv_triple(uint32_t v, uint32_t a, uint32_t b, uint32_t* out)
{
    if (v < a) { out[0] = v; out[1] = a; out[2] = b; }
    else if (v < b) { out[0] = a; out[1] = v; out[2] = b; }
    else { out[0] = a; out[1] = b; out[2] = v; }
}

/* Steps 5 and 6 for ONE target, serial: the unique walk over the sorted triples, the chain, the slots.
 *   keys [n_pairs]: akz_cv_pair_key of the triples at or above the covisibility minimum, ascending; cand [n_cand]: the candidate
 *   views' blocks, ascending; v: the target.  Scratch: visited [n_cand + 1] bytes, unique [(n_pairs + 31) / 32] words.
 *   Slot k < limit gets views[3 k ..], count[k] (the full covisible count, 0 for an unused slot) and start[k], the entries of
 *   the slots in front of it with every list cut to maximum_landmarks; stats [AKZ_CV_STATS] gets its words PAIRS, UNIQUE,
 *   EMITTED and the LIMIT_REACHED flag (the others are the caller's).  -> the target's entries in all.
 * any(|view| already_visited.insert(view)) stops inserting at the first view that is new (lib.rs:2493), and take() stops
 * pulling — and with it inserting — once it has maximum_constraints (lib.rs:2494). */
AKZ_CV_FN uint32_t akz_cv_walk(const uint64_t* keys, uint32_t n_pairs, const uint32_t* cand, uint32_t n_cand, uint32_t v,
                               const akz_cv_settings* st, unsigned char* visited, uint32_t* unique, uint32_t* views, uint32_t* count,
                               uint32_t* start, uint32_t* stats)
{
    uint32_t n_unique = 0u, emitted = 0u, total = 0u, more = 0u;
    for (uint32_t k = 0; k <= n_cand; ++k) visited[k] = 0;
    for (uint32_t k = 0; k < (n_pairs + 31u) / 32u; ++k) unique[k] = 0u;
    for (uint32_t i = 0; i < n_pairs && n_unique < st->maximum_constraints; ++i) {
        uint32_t a, b, order[3];
        akz_cv_pair_from_index(akz_cv_pair_key_index(keys[i]), n_cand, &a, &b);
        /* the triple's views in canonical order, as indices into visited: candidate index, n_cand for the target */
        if (v < cand[a]) { order[0] = n_cand; order[1] = a; order[2] = b; }
        else if (v < cand[b]) { order[0] = a; order[1] = n_cand; order[2] = b; }
        else { order[0] = a; order[1] = b; order[2] = n_cand; }
        for (int k = 0; k < 3; ++k)
            if (!visited[order[k]]) {
                visited[order[k]] = 1;
                unique[i >> 5] |= 1u << (i & 31u);
                ++n_unique;
                break;
            }
    }
    for (int pass = 0; pass < 2; ++pass)                       /* the unique triples, then the rest, both in sorted order */
        for (uint32_t i = 0; i < n_pairs; ++i) {
            if ((((unique[i >> 5] >> (i & 31u)) & 1u) != 0u) != (pass == 0)) continue;
            const uint32_t c = akz_cv_pair_key_count(keys[i]);
            if (c < st->minimum_landmarks) continue;           /* optimize_three_view returns None (lib.rs:1949) */
            if (emitted == st->limit) {
                more = 1u;
                continue;
            }
            uint32_t a, b;
            akz_cv_pair_from_index(akz_cv_pair_key_index(keys[i]), n_cand, &a, &b);
            akz_cv_triple(v, cand[a], cand[b], views + 3 * (size_t)emitted);
            count[emitted] = c;
            start[emitted] = total;
            total += c < st->maximum_landmarks ? c : st->maximum_landmarks;
            ++emitted;
        }
    for (uint32_t k = emitted; k < st->limit; ++k) {
        views[3 * (size_t)k] = views[3 * (size_t)k + 1] = views[3 * (size_t)k + 2] = 0u;
        count[k] = 0u;
        start[k] = total;
    }
    stats[AKZ_CV_S_PAIRS] = n_pairs;
    stats[AKZ_CV_S_UNIQUE] = n_unique;
    stats[AKZ_CV_S_EMITTED] = emitted;
    stats[AKZ_CV_S_FLAGS] |= more ? (uint32_t)AKZ_CV_F_LIMIT_REACHED : 0u;
    return total;
}

/* the views of the reconstruction that holds view v: the first range [graph_start[g], graph_start[g + 1]) with v inside;
 * AKZ_CV_NONE when there is none */
AKZ_CV_FN uint32_t akz_cv_graph_views(const uint32_t* graph_start, uint32_t n_graphs, uint32_t v)
{
    for (uint32_t g = 0; g < n_graphs; ++g)
        if (graph_start[g] <= v && v < graph_start[g + 1]) return graph_start[g + 1] - graph_start[g];
    return AKZ_CV_NONE;
}

/* record_view_constraints for ONE target: verdict [limit] the constraint stage's words of its slots -> recorded [limit], the
 * target's verdict; *n_recorded the constraints recorded.  The first maximum_constraints accepted slots are the
 * .filter_map(..).take(..) of lib.rs:2511-2514; the refusal is lib.rs:2098-2102. */
AKZ_CV_FN int akz_cv_record(const uint32_t* verdict, const akz_cv_settings* st, uint32_t graph_views, uint32_t* recorded, uint32_t* n_recorded)
{
    uint32_t n = 0u;
    for (uint32_t k = 0; k < st->limit; ++k) {
        const int take = verdict[k] == 0u && n < st->maximum_constraints;
        recorded[k] = verdict[k] != 0u ? verdict[k] : take ? 0u : (uint32_t)AKZ_CV_NOT_RECORDED;
        n += take ? 1u : 0u;
    }
    /* constraints.len() + 1 < views.len(), in usize: no wrap for any u32 */
    if (n < st->minimum_new && (uint64_t)n + 1u < (uint64_t)graph_views) {
        for (uint32_t k = 0; k < st->limit; ++k)
            if (recorded[k] == 0u) recorded[k] = (uint32_t)AKZ_CV_NOT_RECORDED;
        *n_recorded = 0u;
        return AKZ_CV_FEW_CONSTRAINTS;
    }
    *n_recorded = n;
    return AKZ_CV_OK;
}

/* flatten_constraints: edge slot s of a constraint has the constraint's view AKZ_CV_SLOT_TARGET(s) as its target
 * (ThreeViewConstraint::edge_constraints, lib.rs:167-180: {0, 0, 1, 1, 2, 2}) */
#define AKZ_CV_SLOT_TARGET(s) ((s) >> 1)

#endif /* AKZ_COVISIBILITY_MATH_H */
