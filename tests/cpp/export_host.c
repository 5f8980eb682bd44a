/* The CPU checker of the export kernels: the host's execution of the whole procedure is in include/akz_export_math.h itself (the
 * kernels' loops of cv_amd/csrc/rs_export.hip one after another, around the decisions and the arithmetic the kernels compile
 * for the device); this file exports it.  tests/export_checker.py has tests/host_build.py build it with the host compiler into
 * a shared object and loads it with ctypes.  Every output buffer is produced whole: what the device call does not write is not
 * written here either, so that both sides can start from one fill.
 */
#include <stddef.h>
#include <stdint.h>

#include "../../include/akz_export_math.h"

/* rs_export_reconstruction_device on host arrays */
void ex_export(const double* world, uint32_t n_world, const uint32_t* start, const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks,
               const unsigned char* colors, const uint32_t* view_blocks, uint32_t n_views, const uint32_t* counts, const uint32_t* landmarks,
               uint32_t cap, uint32_t n_blocks, const double* poses, uint32_t room, double* xyz, unsigned char* rgb, uint32_t* key, double* cameras,
               uint32_t* counts_out, uint32_t* verdict)
{
    akz_ex_export(world, n_world, start, obs, n_obs, n_landmarks, colors, view_blocks, n_views, counts, landmarks, cap, n_blocks, poses, room, xyz,
                  rgb, key, cameras, counts_out, verdict);
}

/* ---- the pieces, for the rule tests ---- */
void ex_camera(const double* pose, double mean, double* cam) { akz_ex_camera(pose, mean, cam); }
void ex_camera_vertex(const double* cam, int k, double* v) { akz_ex_camera_vertex(cam, k, v); }
