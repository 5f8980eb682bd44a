/* akz_triangulate_math.h — cv-geom's Linear-Eigen triangulator and cv-sfm's robustness test around it, written as plain
 * IEEE double arithmetic so that gcc (the CPU checker, tests/cpp/triangulate_host.c) and hipcc (the gfx950 kernels of
 * cv_amd/csrc/rs_triangulate.hip) execute the same operation sequence (build: -ffp-contract=off, no fast-math; sqrt is the
 * one non-arithmetic primitive).  Parity is "host build == HIP", bit for bit.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   LinearEigenTriangulator::triangulate_observations   cv-geom/src/triangulation.rs:82-130
 *   Projective::from_homogeneous                        cv-core/src/point.rs:20-25
 *   TriangulatorObservations::..._to_camera, Relative   cv-core/src/triangulation.rs:21-36, 52-67
 *   VSlam::are_observations_robust                      cv-sfm/src/lib.rs:2895-2934
 *   CameraIntrinsics::calibrate (+K1)                   cv-pinhole/src/lib.rs:108-117, 191-202
 *
 * Unpinned against the reference (nalgebra 0.30 is not vendored in the reference tree):
 *   - the eigen-solver: nalgebra's try_symmetric_eigen (tridiagonalisation + implicit QR) is not restated; both sides use
 *     akz_rm_jacobi4_sym of akz_ransac_math.h.  Agreement with the reference is at the level its own doc-test pins
 *     (distance < 1e-6 on exact data); with LAPACK see tests/test_triangulate_math.py;
 *   - the order of nalgebra's matrix products and of its norm: fixed below, entry by entry, left to right;
 *   - the order of a landmark's observations: the reference walks a HashMap; here it is the order of the caller's list.
 */
#ifndef AKZ_TRIANGULATE_MATH_H
#define AKZ_TRIANGULATE_MATH_H

#include "akz_ransac_math.h"

/* why a row of the table is "None" ({0, 0, 0, -1}); 0 = a point was written */
enum {
    AKZ_TRI_OK = 0,
    AKZ_TRI_TOO_FEW = 1,     /* fewer than 2 observations (triangulation.rs:87-89) */
    AKZ_TRI_NOT_ROBUST = 2,  /* are_observations_robust said no (lib.rs:2907-2934) */
    AKZ_TRI_EIGEN = 3,       /* the eigen-solver did not converge within max_sweeps (try_symmetric_eigen -> None) */
    AKZ_TRI_NOT_FINITE = 4,  /* the design matrix or the point holds a NaN or an infinity (triangulation.rs:117-120) */
    AKZ_TRI_CHEIRALITY = 5,  /* the point lies behind an observing camera (triangulation.rs:121-128) */
    AKZ_TRI_BAD_INDEX = 6    /* an observation names a block, a feature or a landmark outside the caller's arrays */
};

/* true for every ordinary number, false for NaN and the infinities (x - x is 0 exactly then, NaN otherwise) */
#define AKZ_TRI_FINITE(x) (((x) - (x)) == 0.0)

AKZ_RM_FN void akz_tri_none(double* out)
{
    out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = -1.0;
}

/* CameraIntrinsics::calibrate / CameraIntrinsicsK1Distortion::calibrate for one keypoint (cv-pinhole/src/lib.rs:108-117,
 * 191-202): the statement rs_calibrate and the batched consensus use, restated so that the CPU checker shares it.
 * intr = {focal_x, focal_y, principal_x, principal_y, skew}. */
AKZ_RM_FN void akz_tri_calibrate(const double* intr, int use_k1, double k1, float kx, float ky, double* out)
{
    double cx = (double)kx - intr[2], cy = (double)ky - intr[3];
    double y = cy / intr[1];
    double x = (cx - intr[4] * y) / intr[0];
    if (use_k1) {
        double r2 = x * x + y * y;
        double d = 1.0 + k1 * r2;
        x = x / d;
        y = y / d;
    }
    double nrm = AKZ_RM_SQRT(x * x + y * y + 1.0 * 1.0);
    out[0] = x / nrm;
    out[1] = y / nrm;
    out[2] = 1.0 / nrm;
}

/* One observation into the 4 x 4 design matrix (triangulation.rs:91-106): term = P - (b b^T) P (3 x 4), A += term^T term.
 * pose = row-major [R | t] of the WorldToCamera, a[r * 4 + c] with r <= c only (A is symmetric: the lower triangle is
 * never read or written, as akz_rm_jacobi4_sym wants it).  Product order, unpinned: (b b^T)[i][k] = b[i] * b[k] first;
 * every three-term sum is ((x0 + x1) + x2), k ascending. */
AKZ_RM_FN void akz_tri_accumulate(double* a, const double* pose, const double* b)
{
    double term[12];
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double m0 = b[i] * b[0], m1 = b[i] * b[1], m2 = b[i] * b[2];
        AKZ_RM_UNROLL
        for (int c = 0; c < 4; ++c) term[i * 4 + c] = pose[i * 4 + c] - ((m0 * pose[c] + m1 * pose[4 + c]) + m2 * pose[8 + c]);
    }
    AKZ_RM_UNROLL
    for (int r = 0; r < 4; ++r) {
        AKZ_RM_UNROLL
        for (int c = r; c < 4; ++c) a[r * 4 + c] += (term[r] * term[c] + term[4 + r] * term[4 + c]) + term[8 + r] * term[8 + c];
    }
}

/* pose.inverse().isometry() * bearing (triangulation.rs:124-125, lib.rs:2922-2923): the bearing in world axes, R^T b */
AKZ_RM_FN void akz_tri_world_bearing(const double* pose, const double* b, double* d)
{
    AKZ_RM_UNROLL
    for (int j = 0; j < 3; ++j) d[j] = (pose[j] * b[0] + pose[4 + j] * b[1]) + pose[8 + j] * b[2];
}

/* is_bi_observation_angularly_robust (lib.rs:2895-2904) on two world-axes bearings */
AKZ_RM_FN int akz_tri_pair_robust(const double* da, const double* db, double min_cos_distance)
{
    return 1.0 - ((da[0] * db[0] + da[1] * db[1]) + da[2] * db[2]) > min_cos_distance;
}

/* The cheirality test of one observation (triangulation.rs:121-128): (R^T b) . point.bearing() is_sign_positive — the
 * sign BIT, so +0.0 passes and -0.0 does not. */
AKZ_RM_FN int akz_tri_in_front(const double* pose, const double* b, const double* point)
{
    double d[3];
    akz_tri_world_bearing(pose, b, d);
    const double dot = (d[0] * point[0] + d[1] * point[1]) + d[2] * point[2];
    return !__builtin_signbit(dot);
}

/* float_ord::FloatOrd's key: the SIGNED total order of the bit patterns (-NaN < -inf < .. < -0.0 < +0.0 < .. < +inf <
 * +NaN).  Not the abs().to_bits() key of cv-core/src/pose.rs:282 that CameraToCamera::residual selects with. */
AKZ_RM_FN unsigned long long akz_tri_float_ord(double x)
{
    unsigned long long u;
    __builtin_memcpy(&u, &x, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

/* Projective::from_homogeneous (cv-core/src/point.rs:20-25), in place: the whole vector is negated when w
 * is_sign_negative — the sign BIT, so w = -0.0 negates too and comes out as +0.0 — then all four are divided by
 * |xyz| = sqrt((x^2 + y^2) + z^2). */
AKZ_RM_FN void akz_tri_from_homogeneous(double* p)
{
    if (__builtin_signbit(p[3])) {
        p[0] = -p[0]; p[1] = -p[1]; p[2] = -p[2]; p[3] = -p[3];
    }
    const double nrm = AKZ_RM_SQRT((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
    p[0] = p[0] / nrm; p[1] = p[1] / nrm; p[2] = p[2] / nrm; p[3] = p[3] / nrm;
}

/* From the finished design matrix to the point (triangulation.rs:108-120): eigen-decomposition, the eigenvector of the
 * smallest eigenvalue by FloatOrd (the first of equal keys, as Iterator::min_by_key), Projective::from_homogeneous
 * (akz_tri_from_homogeneous), the finite filter.  a is destroyed.  A design matrix that is not finite is refused before the solver (the reference's
 * solver would run out of iterations on it: None either way).  The solver "fails" when it has not met its stopping rule
 * within max_sweeps tests of it.  Returns an AKZ_TRI_* reason; out = the point or "None". */
AKZ_RM_FN int akz_tri_solve(double* a, double eps, int max_sweeps, double* out)
{
    double v[16];
    int fin = 1;
    AKZ_RM_UNROLL
    for (int r = 0; r < 4; ++r) {
        AKZ_RM_UNROLL
        for (int c = r; c < 4; ++c) fin = fin && AKZ_TRI_FINITE(a[r * 4 + c]);
    }
    akz_tri_none(out);
    if (!fin) return AKZ_TRI_NOT_FINITE;
    if (akz_rm_jacobi4_sym(a, v, eps, max_sweeps) >= max_sweeps) return AKZ_TRI_EIGEN;
    unsigned long long best = akz_tri_float_ord(a[0]);
    double p[4] = {v[0], v[4], v[8], v[12]};
    AKZ_RM_UNROLL
    for (int k = 1; k < 4; ++k) {
        const unsigned long long key = akz_tri_float_ord(a[k * 4 + k]);
        if (key < best) {
            best = key;
            p[0] = v[k]; p[1] = v[4 + k]; p[2] = v[8 + k]; p[3] = v[12 + k];
        }
    }
    akz_tri_from_homogeneous(p);
    if (!(AKZ_TRI_FINITE(p[0]) && AKZ_TRI_FINITE(p[1]) && AKZ_TRI_FINITE(p[2]) && AKZ_TRI_FINITE(p[3]))) return AKZ_TRI_NOT_FINITE;
    out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = p[3];
    return AKZ_TRI_OK;
}

/* The settings of one call (rs_triangulate_params of include/akz.h without its size field). */
typedef struct akz_tri_settings {
    double eps;                               /* LinearEigenTriangulator::epsilon, 1e-12 */
    int max_sweeps;                           /* LinearEigenTriangulator::max_iterations, 1000 */
    unsigned robust_minimum_observations;     /* cv-sfm/src/settings.rs:344-350: 3 */
    unsigned n_views;                         /* views of the reconstruction, for the min() of lib.rs:2913-2917 */
    double incidence_minimum_cosine_distance; /* 1e-3 */
} akz_tri_settings;

/* The whole procedure for ONE list of observations, for any source of observations: NAME(src, n, robust, settings, out)
 * with FETCH(src, i, pose[12], bearing[3]) -> 0 when observation i names something outside the caller's arrays (reason 6,
 * nothing is read out of bounds), 1 otherwise.  The host checker fetches from arrays, the kernels gather
 * {block, feature} -> keypoint -> bearing and the block's pose: the text between the fetches is the same.
 *
 * robust != 0 (triangulate_landmark_robust / triangulate_merged_landmark_robust, lib.rs:2958-3000):
 * are_observations_robust first — n >= min(robust_minimum_observations, n_views) and SOME pair i < j with
 * 1 - (R_i^T b_i) . (R_j^T b_j) > incidence_minimum_cosine_distance.  "Some pair" is a disjunction: its value does not
 * depend on the order the pairs are tried in, so the pairs (0, j) are tried while the design matrix is accumulated (the
 * common case ends there) and only a list where none of them passes pays for the other pairs, with observations fetched
 * again instead of kept (a list may be longer than any register file).
 * Precedence of the reasons: 6, 1, 2, then 4 / 3 / 4 of akz_tri_solve, 5. */
#define AKZ_TRI_DEFINE_TRIANGULATE(NAME, SRC_T, FETCH)                                                                   \
    AKZ_RM_FN int NAME(const SRC_T* src, unsigned n, int robust, const akz_tri_settings* st, double* out)                \
    {                                                                                                                    \
        double a[16], pose[12], b[3], d0[3] = {0.0, 0.0, 0.0}, d[3], p[4];                                               \
        int pair_ok = 0;                                                                                                 \
        AKZ_RM_UNROLL                                                                                                    \
        for (int k = 0; k < 16; ++k) a[k] = 0.0;                                                                         \
        akz_tri_none(out);                                                                                               \
        for (unsigned i = 0; i < n; ++i) {                                                                               \
            if (!FETCH(src, i, pose, b)) return AKZ_TRI_BAD_INDEX;                                                       \
            akz_tri_accumulate(a, pose, b);                                                                              \
            if (robust) {                                                                                                \
                akz_tri_world_bearing(pose, b, d);                                                                       \
                if (i == 0) {                                                                                            \
                    d0[0] = d[0]; d0[1] = d[1]; d0[2] = d[2];                                                            \
                } else if (!pair_ok)                                                                                     \
                    pair_ok = akz_tri_pair_robust(d0, d, st->incidence_minimum_cosine_distance);                         \
            }                                                                                                            \
        }                                                                                                                \
        if (n < 2u) return AKZ_TRI_TOO_FEW;                                                                              \
        if (robust) {                                                                                                    \
            const unsigned need = st->robust_minimum_observations < st->n_views ? st->robust_minimum_observations        \
                                                                                 : st->n_views;                          \
            if (n < need) return AKZ_TRI_NOT_ROBUST;                                                                     \
            for (unsigned i = 1; i + 1u < n && !pair_ok; ++i) {                                                          \
                FETCH(src, i, pose, b);                                                                                  \
                akz_tri_world_bearing(pose, b, d0);                                                                      \
                for (unsigned j = i + 1u; j < n && !pair_ok; ++j) {                                                      \
                    FETCH(src, j, pose, b);                                                                              \
                    akz_tri_world_bearing(pose, b, d);                                                                   \
                    pair_ok = akz_tri_pair_robust(d0, d, st->incidence_minimum_cosine_distance);                         \
                }                                                                                                        \
            }                                                                                                            \
            if (!pair_ok) return AKZ_TRI_NOT_ROBUST;                                                                     \
        }                                                                                                                \
        const int why = akz_tri_solve(a, st->eps, st->max_sweeps, p);                                                    \
        if (why != AKZ_TRI_OK) return why;                                                                               \
        for (unsigned i = 0; i < n; ++i) {                                                                               \
            FETCH(src, i, pose, b);                                                                                      \
            if (!akz_tri_in_front(pose, b, p)) return AKZ_TRI_CHEIRALITY;                                                \
        }                                                                                                                \
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2]; out[3] = p[3];                                                      \
        return AKZ_TRI_OK;                                                                                               \
    }

#endif /* AKZ_TRIANGULATE_MATH_H */
