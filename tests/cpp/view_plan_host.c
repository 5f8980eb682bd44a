/* The CPU checker of the view-plan kernels: the host's execution of a call is in include/akz_view_plan_math.h itself (the kernels'
 * steps of cv_amd/csrc/hm_view_plan.hip one after another, around the decisions the kernels compile for the device); this file
 * hands it a call's arrays.  tests/test_view_plan_math.py has tests/host_build.py build it with the host compiler into a shared
 * object and loads it with ctypes.
 */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_view_plan_math.h"

/* hm_view_plan_device on host arrays; -1: no memory */
int vp_plan(const uint32_t* views_out, const uint32_t* group_recon, const uint32_t* group_start, const uint32_t* counts, const uint32_t* find_verdict,
            uint32_t room, const uint32_t* pick, uint32_t flags, uint32_t n_frames, uint32_t n_views, uint32_t n_blocks, uint32_t exp_blocks,
            uint32_t* view_idx, uint32_t* frame_views, uint32_t* verdict, uint32_t* plan_counts)
{
    uint32_t* flag = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)n_blocks + 1));
    if (!flag) return -1;
    akz_vp_plan(views_out, group_recon, group_start, counts, find_verdict, room, pick, flags, n_frames, n_views, n_blocks, exp_blocks, view_idx,
                frame_views, verdict, plan_counts, flag);
    free(flag);
    return 0;
}

/* ---- the pieces, for the rule tests ---- */
uint32_t vp_group_by_ordinal(int has_pick, uint32_t pick, uint32_t n_groups) { return akz_vp_group_by_ordinal(has_pick, pick, n_groups); }
uint32_t vp_group_span(uint32_t start_word, uint32_t end_word, uint32_t room, uint32_t* start) { return akz_vp_group_span(start_word, end_word, room, start); }
uint32_t vp_taken(uint32_t length, uint32_t n_views) { return akz_vp_taken(length, n_views); }
uint32_t vp_list_verdict(uint32_t length, uint32_t n_views) { return akz_vp_list_verdict(length, n_views); }
uint32_t vp_call_verdict(uint32_t distinct, uint32_t exp_blocks) { return akz_vp_call_verdict(distinct, exp_blocks); }
int vp_live(uint32_t v, uint32_t frame_views, uint32_t n_views, uint32_t key, uint32_t n_blocks) { return akz_vp_live(v, frame_views, n_views, key, n_blocks); }
