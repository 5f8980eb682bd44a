/* akz_repack_math.h — the repacking of a reconstruction: views removed, the landmark table compacted, rows and blocks
 * renumbered.  Integer decisions only, written once for gcc (the CPU checker, tests/cpp/repack_host.c) and hipcc (the gfx950
 * kernels of cv_amd/csrc/rs_repack.hip): parity is "host build == HIP" in every byte of every output.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlamData::remove_view                   cv-sfm/src/lib.rs:517-546
 *   its callers: apply_bundle_adjust         cv-sfm/src/lib.rs:502-515
 *                incorporate_reconstruction  cv-sfm/src/lib.rs:1880-1884
 *                try_merge_reconstructions   cv-sfm/src/lib.rs:2147
 *
 * Departures:
 *   - the reference removes one view at a time from slotmaps whose keys never move; a call here removes every view the block map
 *     marks at once (a landmark goes when its last observation goes, so the order of removal cannot matter) and then renumbers:
 *     kept rows leave in ascending old key (stable), a row's kept observations keep their order, blocks go through the map;
 *   - remove_view panics on a landmark without observations; here such a row (a tombstone of merge_landmarks, the empty tail
 *     behind rs_add_views_device's filled rows) is dropped and counted;
 *   - a call that is refused (a broken table, map or index, or rooms too small) describes an EMPTY table in every output
 *     rather than a partial one: the caller still holds the old generation;
 *   - the constraints are compacted in order (the reference's retain over a slotmap has no order); the room behind the count
 *     holds triples no stage takes (views 0xFFFFFFFF, verdict RS_TVC_BAD_INDEX, poses 0), so that the room can be passed on as
 *     the count without a read-back.
 */
#ifndef AKZ_REPACK_MATH_H
#define AKZ_REPACK_MATH_H

#include <stddef.h>
#include <stdint.h>

#include "akz_landmark_table_math.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define AKZ_RP_FN __host__ __device__ static inline
#else
#define AKZ_RP_FN static inline
#endif

/* the verdict on a call (RS_RP_* of include/akz.h) */
enum {
    AKZ_RP_OK = 0,
    AKZ_RP_BAD_TABLE = 1,      /* the starts do not ascend inside [0, n_obs], or the range starts do not inside [0, n_landmarks] */
    AKZ_RP_BAD_INDEX = 2,      /* an observation of a row names a block >= n_blocks, or a kept one a feature >= cap */
    AKZ_RP_BAD_MAP = 3,        /* a map entry that is neither removed nor below n_blocks_out, or two blocks with one target */
    AKZ_RP_NO_ROOM = 4         /* more kept rows than lm_room or more kept observations than obs_room */
};
/* words of d_counts_out */
enum {
    AKZ_RP_C_ROWS = 0,            /* rows kept */
    AKZ_RP_C_OBSERVATIONS = 1,    /* observations kept */
    AKZ_RP_C_EMPTY_DROPPED = 2,   /* rows dropped that were empty */
    AKZ_RP_C_ROWS_DROPPED = 3,    /* rows dropped because every observation was in a removed view */
    AKZ_RP_C_OBS_DROPPED = 4,     /* observations dropped */
    AKZ_RP_COUNTS = 5
};
enum { AKZ_RP_TVC_BAD_INDEX = 3 };   /* RS_TVC_BAD_INDEX: the verdict of the constraint slots behind the count */
#define AKZ_RP_NONE 0xFFFFFFFFu

/* the new block of old block b < n_blocks; map == NULL is the identity */
AKZ_RP_FN uint32_t akz_rp_map(const uint32_t* map, uint32_t b) { return map ? map[b] : b; }

/* a map entry that names no target: neither "removed" nor a block of the output */
AKZ_RP_FN int akz_rp_entry_bad(uint32_t m, uint32_t n_blocks_out) { return m != AKZ_RP_NONE && m >= n_blocks_out; }

/* a target's reference count after block b took it: a second taker breaks the map */
AKZ_RP_FN int akz_rp_target_shared(uint32_t refs_before) { return refs_before != 0u; }

/* Row l of the table can be walked: its own range ascends inside [0, n_obs] (whatever the rest of the table does). */
AKZ_RP_FN int akz_rp_row_range(const uint32_t* start, uint32_t l, uint32_t n_obs, uint32_t* s, uint32_t* e)
{
    *s = start[l];
    *e = start[l + 1];
    return *s <= *e && *e <= n_obs;
}

/* What observation {blk, feat} does: 0 dropped, 1 kept, -1 a bad index. */
AKZ_RP_FN int akz_rp_observation(const uint32_t* map, uint32_t blk, uint32_t feat, uint32_t n_blocks, uint32_t cap)
{
    if (blk >= n_blocks) return -1;
    if (akz_rp_map(map, blk) == AKZ_RP_NONE) return 0;
    return feat < cap ? 1 : -1;
}

/* range start r <= n_recons breaks "the range starts ascend inside [0, n_landmarks]" */
AKZ_RP_FN int akz_rp_range_bad(const uint32_t* recon_start, uint32_t r, uint32_t n_recons, uint32_t n_landmarks)
{
    return r < n_recons ? recon_start[r] > recon_start[r + 1] : recon_start[r] > n_landmarks;
}

/* The call's verdict from what the passes found.  One order for both builds: table, map, index, room. */
AKZ_RP_FN uint32_t akz_rp_verdict(int bad_table, int bad_map, int bad_index, uint32_t rows, uint32_t observations, uint32_t lm_room,
                                  uint32_t obs_room)
{
    if (bad_table) return AKZ_RP_BAD_TABLE;
    if (bad_map) return AKZ_RP_BAD_MAP;
    if (bad_index) return AKZ_RP_BAD_INDEX;
    return (rows > lm_room || observations > obs_room) ? AKZ_RP_NO_ROOM : AKZ_RP_OK;
}

/* d_counts_out holds the true numbers for a table that could be counted (OK and NO_ROOM), zeros otherwise */
AKZ_RP_FN int akz_rp_counted(uint32_t verdict) { return verdict == AKZ_RP_OK || verdict == AKZ_RP_NO_ROOM; }

/* A constraint is kept iff all three of its views are views of the input that the map keeps (remove_view's retain).  A view
 * >= n_blocks or an entry that names no block of the output drops the constraint too: nothing is read out of bounds and no
 * view >= n_blocks_out leaves in front of the count. */
AKZ_RP_FN int akz_rp_constraint_kept(const uint32_t* map, const uint32_t* views3, uint32_t n_blocks, uint32_t n_blocks_out)
{
    for (int k = 0; k < 3; ++k) {
        if (views3[k] >= n_blocks) return 0;
        if (akz_rp_map(map, views3[k]) >= n_blocks_out) return 0;       /* AKZ_RP_NONE included */
    }
    return 1;
}

/* What becomes of {recon, view} of a stored frame under the map of reconstruction `recon`: 0 untouched, 1 the view is mapped
 * (*view_out), 2 the frame loses its view (remove_view's frame.view = None), -1 untouched and flagged (view >= n_blocks). */
AKZ_RP_FN int akz_rp_frame(const uint32_t* map, uint32_t frame_recon, uint32_t frame_view, uint32_t recon, uint32_t n_blocks,
                           uint32_t* view_out)
{
    if (frame_recon != recon || recon == AKZ_RP_NONE) return 0;
    if (frame_view >= n_blocks) return -1;
    *view_out = akz_rp_map(map, frame_view);
    return *view_out == AKZ_RP_NONE ? 2 : 1;
}

#endif /* AKZ_REPACK_MATH_H */
