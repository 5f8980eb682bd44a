/* akz_view_plan_math.h — from the frames a frame was found to be compared with to the views it is matched against: which of the
 * found reconstructions a frame takes, how many of that reconstruction's views, which frames are refused, and how many distinct
 * view blocks a whole micro-batch searches.  All of it is integers.  Written once for gcc (the CPU checker,
 * tests/cpp/view_plan_host.c) and hipcc (the gfx950 kernels of cv_amd/csrc/hm_view_plan.hip): parity is "host build == HIP" in
 * every byte of every output.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   try_localize: one reconstruction per turn of the loop, most views found first   cv-sfm/src/lib.rs:858-891
 *   try_localize_and_incorporate: .remove(&reconstruction), the named group alone   cv-sfm/src/lib.rs:926-939
 *   register_frame_subset: walks exactly the list it was handed                      cv-sfm/src/lib.rs:1472-1486
 *
 * Inputs per frame f: row f of the outputs of hm_find_frames_batch_device (views_out, group_recon: pitch `room`; group_start:
 * pitch room + 1; counts: AKZ_PL_COUNTS; verdict) and an optional pick word.
 *
 * Departures:
 *   - a group longer than n_views is cut to its first n_views keys (AKZ_VP_CUT); the reference walks the whole list.  With
 *     n_views = hm_place_room(params) <= 64 nothing is cut;
 *   - a view key is a block of the descriptor table; a taken key >= n_blocks refuses its frame alone (AKZ_VP_BAD_VIEW);
 *   - more distinct blocks than the caller left room for refuse the call (AKZ_VP_NO_ROOM): nothing is searched.
 */
#ifndef AKZ_VIEW_PLAN_MATH_H
#define AKZ_VIEW_PLAN_MATH_H

#include <stddef.h>
#include <stdint.h>

#include "akz_place_math.h"

#ifndef AKZ_RM_FN
#if defined(__HIPCC__) || defined(__HIP__)
#define AKZ_RM_FN __host__ __device__ static inline
#else
#define AKZ_RM_FN static inline
#endif
#endif

/* the verdict on a frame, and (OK or NO_ROOM) on the call (HM_VP_* of include/akz.h) */
enum {
    AKZ_VP_OK = 0,
    AKZ_VP_CUT = 1,             /* the group was longer than n_views: its first n_views keys were taken */
    AKZ_VP_NO_GROUP = 2,        /* no group of that ordinal / reconstruction key, or the find had no groups */
    AKZ_VP_FIND_REFUSED = 3,    /* the find's verdict for the query is not AKZ_PL_OK: nothing of its rows is read */
    AKZ_VP_BAD_VIEW = 4,        /* a taken view key >= n_blocks: nothing is read through it */
    AKZ_VP_NO_ROOM = 5          /* the call's: more distinct target blocks than exp_blocks */
};
/* words of d_plan_counts */
enum { AKZ_VP_C_BLOCKS = 0, AKZ_VP_C_LIVE = 1, AKZ_VP_C_VERDICT = 2, AKZ_VP_C_FRAMES = 3, AKZ_VP_COUNTS = 4 };
/* call flags */
enum { AKZ_VP_PICK_RECON = 1 };  /* d_pick holds reconstruction keys, not ordinals */
/* the limit of n_views (the best-of-views kernel's) */
enum { AKZ_VP_MAX_VIEWS = 64 };

/* ---- which group ---- */
/* the groups of a find row that may be looked at: the row holds `room` words */
AKZ_RM_FN uint32_t akz_vp_groups(uint32_t n_groups, uint32_t room) { return n_groups < room ? n_groups : room; }
/* pick by ordinal (has_pick 0: the first turn of the loop, the reconstruction with most views found): the group, or AKZ_PL_NONE */
AKZ_RM_FN uint32_t akz_vp_group_by_ordinal(int has_pick, uint32_t pick, uint32_t n_groups)
{
    const uint32_t g = has_pick ? pick : 0u;
    return g < n_groups ? g : AKZ_PL_NONE;
}
/* pick by key: is group g, whose reconstruction is `recon`, the one .remove(&pick) takes? (the keys of a row are distinct) */
AKZ_RM_FN int akz_vp_group_is(uint32_t recon, uint32_t pick) { return recon == pick; }

/* ---- its list ---- */
/* a group's place in the row, held inside the row whatever the words say: [*start, *start + length) with start + length <= room */
AKZ_RM_FN uint32_t akz_vp_group_span(uint32_t start_word, uint32_t end_word, uint32_t room, uint32_t* start)
{
    const uint32_t e = end_word < room ? end_word : room, s = start_word < e ? start_word : e;
    *start = s;
    return e - s;
}
/* take(V) */
AKZ_RM_FN uint32_t akz_vp_taken(uint32_t length, uint32_t n_views) { return length < n_views ? length : n_views; }
AKZ_RM_FN uint32_t akz_vp_list_verdict(uint32_t length, uint32_t n_views) { return length > n_views ? (uint32_t)AKZ_VP_CUT : (uint32_t)AKZ_VP_OK; }
AKZ_RM_FN int akz_vp_key_ok(uint32_t key, uint32_t n_blocks) { return key < n_blocks; }
/* does a frame's verdict leave it a list? */
AKZ_RM_FN int akz_vp_accepted(uint32_t verdict) { return verdict == (uint32_t)AKZ_VP_OK || verdict == (uint32_t)AKZ_VP_CUT; }

/* ---- the call ---- */
AKZ_RM_FN uint32_t akz_vp_call_verdict(uint32_t distinct, uint32_t exp_blocks) { return distinct > exp_blocks ? (uint32_t)AKZ_VP_NO_ROOM : (uint32_t)AKZ_VP_OK; }
/* problem (f, v) of a planned search: is it searched?  (a list written by anything else than the plan is held to the same tests) */
AKZ_RM_FN int akz_vp_live(uint32_t v, uint32_t frame_views, uint32_t n_views, uint32_t key, uint32_t n_blocks)
{
    return v < akz_vp_taken(frame_views, n_views) && akz_vp_key_ok(key, n_blocks);
}

/* ---- the host's execution (the kernels' steps of hm_view_plan.hip one after another) ---- */
/* One frame: its row of view_idx (n_views words, the entries behind the list AKZ_PL_NONE), its count and its verdict. */
AKZ_RM_FN void akz_vp_pick_one(const uint32_t* views_out, const uint32_t* group_recon, const uint32_t* group_start, const uint32_t* counts,
                               uint32_t find_verdict, uint32_t room, int has_pick, uint32_t pick, uint32_t flags, uint32_t n_views,
                               uint32_t n_blocks, uint32_t* view_idx, uint32_t* frame_views, uint32_t* verdict)
{
    for (uint32_t v = 0; v < n_views; ++v) view_idx[v] = AKZ_PL_NONE;
    *frame_views = 0u;
    if (find_verdict != (uint32_t)AKZ_PL_OK) {
        *verdict = AKZ_VP_FIND_REFUSED;
        return;
    }
    const uint32_t n_groups = akz_vp_groups(counts[AKZ_PL_C_GROUPS], room);
    uint32_t g = AKZ_PL_NONE;
    if (has_pick && (flags & (uint32_t)AKZ_VP_PICK_RECON)) {
        for (uint32_t k = 0; k < n_groups && g == AKZ_PL_NONE; ++k)
            if (akz_vp_group_is(group_recon[k], pick)) g = k;
    } else {
        g = akz_vp_group_by_ordinal(has_pick, pick, n_groups);
    }
    if (g == AKZ_PL_NONE) {
        *verdict = AKZ_VP_NO_GROUP;
        return;
    }
    uint32_t start;
    const uint32_t length = akz_vp_group_span(group_start[g], group_start[g + 1u], room, &start);
    const uint32_t taken = akz_vp_taken(length, n_views);
    for (uint32_t v = 0; v < taken; ++v)
        if (!akz_vp_key_ok(views_out[start + v], n_blocks)) {
            *verdict = AKZ_VP_BAD_VIEW;
            return;
        }
    for (uint32_t v = 0; v < taken; ++v) view_idx[v] = views_out[start + v];
    *frame_views = taken;
    *verdict = akz_vp_list_verdict(length, n_views);
}

/* hm_view_plan_device on host arrays.  flag: n_blocks words of scratch.  d_pick null: no pick. */
AKZ_RM_FN void akz_vp_plan(const uint32_t* views_out, const uint32_t* group_recon, const uint32_t* group_start, const uint32_t* counts,
                           const uint32_t* find_verdict, uint32_t room, const uint32_t* pick, uint32_t flags, uint32_t n_frames, uint32_t n_views,
                           uint32_t n_blocks, uint32_t exp_blocks, uint32_t* view_idx, uint32_t* frame_views, uint32_t* verdict,
                           uint32_t* plan_counts, uint32_t* flag)
{
    for (uint32_t b = 0; b < n_blocks; ++b) flag[b] = 0u;
    for (uint32_t f = 0; f < n_frames; ++f) {
        akz_vp_pick_one(views_out + (size_t)f * room, group_recon + (size_t)f * room, group_start + (size_t)f * (room + 1u),
                        counts + (size_t)f * AKZ_PL_COUNTS, find_verdict[f], room, pick != 0, pick ? pick[f] : 0u, flags, n_views, n_blocks,
                        view_idx + (size_t)f * n_views, frame_views + f, verdict + f);
        for (uint32_t v = 0; v < n_views; ++v)
            if (akz_vp_live(v, frame_views[f], n_views, view_idx[(size_t)f * n_views + v], n_blocks)) flag[view_idx[(size_t)f * n_views + v]] = 1u;
    }
    uint32_t distinct = 0u, live = 0u, frames = 0u;
    for (uint32_t b = 0; b < n_blocks; ++b) distinct += flag[b];
    const uint32_t call = akz_vp_call_verdict(distinct, exp_blocks);
    for (uint32_t f = 0; f < n_frames; ++f) {
        if (call != (uint32_t)AKZ_VP_OK) {
            for (uint32_t v = 0; v < n_views; ++v) view_idx[(size_t)f * n_views + v] = AKZ_PL_NONE;
            frame_views[f] = 0u;
        }
        live += frame_views[f];
        frames += frame_views[f] != 0u;
    }
    plan_counts[AKZ_VP_C_BLOCKS] = distinct;
    plan_counts[AKZ_VP_C_LIVE] = live;
    plan_counts[AKZ_VP_C_VERDICT] = call;
    plan_counts[AKZ_VP_C_FRAMES] = frames;
}

#endif /* AKZ_VIEW_PLAN_MATH_H */
