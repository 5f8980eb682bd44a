/* akz_five_point_math.h — the five-point essential-matrix solver (nister-stewenius), written as plain IEEE double
 * arithmetic so that gcc (the CPU checker, tests/cpp/five_point_host.c) and hipcc (the gfx950 kernels of
 * cv_amd/csrc/rs_ransac.hip) execute the same operation sequence (build: -ffp-contract=off, no fast-math; sqrt is the one
 * non-arithmetic primitive).  Parity is "host build == HIP", bit for bit; agreement with an independent float64 statement
 * (tests/five_point_statement.py, LAPACK) is measured in tests/test_five_point_math.py.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   encode_epipolar_equation, five_points_nullspace_basis    nister-stewenius/src/lib.rs:50-96
 *   o1, o2, five_points_polynomial_constraints               nister-stewenius/src/lib.rs:98-204
 *   five_points_relative_pose (elimination, action matrix)   nister-stewenius/src/lib.rs:241-280
 *   essentials_from_action_ebasis                            nister-stewenius/src/lib.rs:219-237
 *
 * ONE DELIBERATE DIFFERENCE.  lib.rs:230 takes `v.fixed_rows::<4>(5)` of the action matrix's eigenvector: rows 5..8.  The
 * monomial order of columns 10..19 is xx xy yy xz yz zz x y z 1 (lib.rs:25-34) and the -1 rows of lib.rs:274-277 tie
 * entry 6 to entry 0, 7 to 1, 8 to 3 and 9 to 6: the coordinates (x, y, z, 1) are rows 6..9.  With rows 5..8 the true
 * essential matrix is among the solutions in 0 of 512 exact synthetic scenes (the cubic constraint is missed by up to
 * 0.97); with rows 6..9 in 512 of 512, to 1.1e-9.  The crate's only integration test is commented out
 * (nister-stewenius/tests/manual.rs).  The specification is therefore lib.rs:50-280 WITH ROWS 6..9.
 *
 * Unpinned against the reference (nalgebra 0.30 is not vendored in the reference tree), fixed here:
 *   - the symmetric eigen-solver of the null space: akz_rm_jacobi9_sym of akz_ransac_math.h, with the stopping rule
 *     AKZ_FP_JACOBI_EPS = 1e-16 instead of NisterStewenius::epsilon = 1e-12.  The reference's 1e-12 is nalgebra's
 *     per-element deflation test; the Jacobi rule bounds the off-diagonal NORM relative to the diagonal's, and a null
 *     vector is mixed with the fifth eigenvector by (off-diagonal element) / (fifth eigenvalue).  On exact data the
 *     fifth eigenvalue is as small as 1.7e-6, so 1e-12 leaves the basis accurate to 1e-6 only (the true E was missed
 *     by up to 8.4e-6 on the 512 seeded scenes of the tests, 2.3e-10 with 1e-16).  The iteration converges
 *     quadratically: the tighter rule costs one more sweep;
 *   - the summation order of the normal matrix: entry by entry, the five rows in ascending order, starting from +0;
 *   - `full_piv_lu().solve()`: Gauss-Jordan elimination with PARTIAL pivoting — in column k the pivot is the row
 *     r >= k of largest |m[r][k]|, the first of equal ones; a pivot that is zero or not finite rejects the sample;
 *   - `complex_eigenvalues()`: reduction to Hessenberg form by stabilised elementary transformations (pivot: first
 *     largest magnitude), then the Francis double-shift QR iteration, at most 30 iterations per eigenvalue (60 in all
 *     is never approached on real data; a sample that reaches the bound is rejected) with the customary exceptional
 *     shifts at iterations 10 and 20.  An eigenvalue is real when the iteration deflates it as a 1 x 1 block or as a
 *     2 x 2 block with non-negative discriminant.  The solutions are emitted in ASCENDING ORDER OF EIGENVALUE
 *     (insertion sort, stable), packed from slot 0;
 *   - the eigenvector (SVD with a 1e-12 null threshold in the reference): the null vector of At - lambda I by Gaussian
 *     elimination with COMPLETE pivoting (first largest magnitude, rows before columns): the last pivot is taken as
 *     zero, its unknown set to one, the others follow by back substitution; the vector is scaled to unit length.
 *     The sign is whatever comes out; the four poses of an essential matrix do not depend on it as a set.
 *
 * Storage.  Everything indexed at run time lives in the caller's workspace w (AKZ_FP_WORK doubles, element k at
 * w[k * S]): the host passes S = 1, a kernel passes an LDS region with S = lanes so that a wave's accesses do not
 * collide.  Private arrays are indexed by compile-time constants only (AKZ_RM_UNROLL), so the device needs no scratch.
 */
#ifndef AKZ_FIVE_POINT_MATH_H
#define AKZ_FIVE_POINT_MATH_H

#include "akz_ransac_math.h"

#define AKZ_FP_EIGEN_THRESHOLD 1e-12 /* lib.rs:38 */
#define AKZ_FP_JACOBI_EPS 1e-16      /* the eps every caller passes (see above) */
#define AKZ_FP_JACOBI_SWEEPS 1000    /* NisterStewenius::iterations */
#define AKZ_FP_QR_ITERS 30           /* Francis iterations per eigenvalue */
#define AKZ_FP_WORK 240              /* doubles of workspace: 200 (10 x 20 matrix), 10 + 10 (eigenvalues), 10 + 10 (permutation, vector) */

#define AKZ_FP_FINITE(x) (((x) - (x)) == 0.0)
#define AKZ_FP_ABS(x) ((x) < 0.0 ? -(x) : (x))

/* ---- step 1: the null space (lib.rs:50-96).  a5 / b5: five unit bearings each, [5][3].  basis[r * 4 + c] = component r
 * of the c-th null vector (NullspaceMat, 9 x 4).  Registers only on the device.  Returns 1, or 0 when the sample is
 * rejected: the eigen-solver did not converge within max_sweeps, something is not finite, or the number of eigenvalues
 * <= 1e-12 is not exactly four. */
AKZ_RM_FN int akz_fp_nullspace(const double* a5, const double* b5, double eps, int max_sweeps, double* basis)
{
    double M[81], V[81];
    AKZ_RM_UNROLL
    for (int i = 0; i < 81; ++i) M[i] = 0.0;
    AKZ_RM_UNROLL
    for (int i = 0; i < 5; ++i) {
        double A[9];
        AKZ_RM_UNROLL
        for (int j = 0; j < 3; ++j) {
            AKZ_RM_UNROLL
            for (int k = 0; k < 3; ++k) A[3 * j + k] = a5[3 * i + j] * b5[3 * i + k];
        }
        AKZ_RM_UNROLL
        for (int r = 0; r < 9; ++r) {
            AKZ_RM_UNROLL
            for (int c = r; c < 9; ++c) M[r * 9 + c] += A[r] * A[c];
        }
    }
    int fin = 1;
    AKZ_RM_UNROLL
    for (int r = 0; r < 9; ++r) {
        AKZ_RM_UNROLL
        for (int c = r; c < 9; ++c) fin = fin && AKZ_FP_FINITE(M[r * 9 + c]);
    }
    if (!fin) return 0;
    if (akz_rm_jacobi9_sym(M, V, eps, max_sweeps) >= max_sweeps) return 0;
    int null_count = 0;
    AKZ_RM_UNROLL
    for (int i = 0; i < 9; ++i) {
        fin = fin && AKZ_FP_FINITE(M[i * 9 + i]);
        null_count += (M[i * 9 + i] <= AKZ_FP_EIGEN_THRESHOLD) ? 1 : 0;
    }
    if (!fin || null_count != 4) return 0;
    /* the four smallest eigenvalues in ascending order, the first minimum on ties, selected without a runtime index */
    unsigned taken = 0u;
    AKZ_RM_UNROLL
    for (int c = 0; c < 4; ++c) {
        double bestv = 0.0;
        int have = 0;
        unsigned pick = 0u;
        double ev[9];
        AKZ_RM_UNROLL
        for (int e = 0; e < 9; ++e) ev[e] = 0.0;
        AKZ_RM_UNROLL
        for (int i = 0; i < 9; ++i) {
            const int take = !((taken >> i) & 1u) && (!have || M[i * 9 + i] < bestv);
            bestv = take ? M[i * 9 + i] : bestv;
            pick = take ? (1u << i) : pick;
            have = have || take;
            AKZ_RM_UNROLL
            for (int e = 0; e < 9; ++e) ev[e] = take ? V[e * 9 + i] : ev[e];
        }
        taken |= pick;
        AKZ_RM_UNROLL
        for (int e = 0; e < 9; ++e) basis[e * 4 + c] = ev[e];
    }
    return 1;
}

/* ---- step 2: the polynomial products (lib.rs:98-136).  Monomial order of a 20-vector (lib.rs:15-34):
 * xxx xxy xyy yyy xxz xyz yyz xzz yzz zzz | xx xy yy xz yz zz x y z 1.  o1's result has entries 10..19 only: it is kept
 * as those ten (q[k] = entry 10 + k). */
AKZ_RM_FN void akz_fp_o1(const double* a, const double* b, double* q)
{
    q[0] = a[0] * b[0];
    q[1] = a[0] * b[1] + a[1] * b[0];
    q[3] = a[0] * b[2] + a[2] * b[0];
    q[2] = a[1] * b[1];
    q[4] = a[1] * b[2] + a[2] * b[1];
    q[5] = a[2] * b[2];
    q[6] = a[0] * b[3] + a[3] * b[0];
    q[7] = a[1] * b[3] + a[3] * b[1];
    q[8] = a[2] * b[3] + a[3] * b[2];
    q[9] = a[3] * b[3];
}

/* a: the ten entries 10..19 of a quadratic (entries 0..9 are zero for every argument the solver passes), b: a linear
 * form (x, y, z, 1); res: all twenty entries */
AKZ_RM_FN void akz_fp_o2(const double* a, const double* b, double* res)
{
    const double xx = a[0], xy = a[1], yy = a[2], xz = a[3], yz = a[4], zz = a[5], x = a[6], y = a[7], z = a[8], one = a[9];
    res[0] = xx * b[0];
    res[1] = xx * b[1] + xy * b[0];
    res[4] = xx * b[2] + xz * b[0];
    res[2] = xy * b[1] + yy * b[0];
    res[5] = xy * b[2] + yz * b[0] + xz * b[1];
    res[7] = xz * b[2] + zz * b[0];
    res[3] = yy * b[1];
    res[6] = yy * b[2] + yz * b[1];
    res[8] = yz * b[2] + zz * b[1];
    res[9] = zz * b[2];
    res[10] = xx * b[3] + x * b[0];
    res[11] = xy * b[3] + x * b[1] + y * b[0];
    res[13] = xz * b[3] + x * b[2] + z * b[0];
    res[12] = yy * b[3] + y * b[1];
    res[14] = yz * b[3] + y * b[2] + z * b[1];
    res[15] = zz * b[3] + z * b[2];
    res[16] = x * b[3] + one * b[0];
    res[17] = y * b[3] + one * b[1];
    res[18] = z * b[3] + one * b[2];
    res[19] = one * b[3];
}

/* o2(o1(p, q) - o1(r, s), e): one of the three terms of the determinant row (lib.rs:154-166) */
AKZ_RM_FN void akz_fp_det_term(const double* p, const double* q, const double* r, const double* s, const double* e, double* res)
{
    double u[10], v[10];
    akz_fp_o1(p, q, u);
    akz_fp_o1(r, s, v);
    AKZ_RM_UNROLL
    for (int k = 0; k < 10; ++k) u[k] = u[k] - v[k];
    akz_fp_o2(u, e, res);
}

/* the 10 x 20 constraint matrix (lib.rs:138-204) from the basis, written to w[(row * 20 + col) * S] */
AKZ_RM_FN void akz_fp_constraints(const double* basis, double* w, int S)
{
    /* e_poly[i][j] = row 3 i + j of the basis: E(i, j) as a linear form in (x, y, z, 1) */
#define AKZ_FP_EP(i, j) (basis + 4 * (3 * (i) + (j)))
    {
        double t0[20], t1[20], t2[20];
        akz_fp_det_term(AKZ_FP_EP(0, 1), AKZ_FP_EP(1, 2), AKZ_FP_EP(0, 2), AKZ_FP_EP(1, 1), AKZ_FP_EP(2, 0), t0);
        akz_fp_det_term(AKZ_FP_EP(0, 2), AKZ_FP_EP(1, 0), AKZ_FP_EP(0, 0), AKZ_FP_EP(1, 2), AKZ_FP_EP(2, 1), t1);
        akz_fp_det_term(AKZ_FP_EP(0, 0), AKZ_FP_EP(1, 1), AKZ_FP_EP(0, 1), AKZ_FP_EP(1, 0), AKZ_FP_EP(2, 2), t2);
        AKZ_RM_UNROLL
        for (int k = 0; k < 20; ++k) w[k * S] = (t0[k] + t1[k]) + t2[k];
    }
    /* E E^T, upper triangle (lib.rs:170-183): L[u] for (i, j) = (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) */
    double L[6][10];
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        AKZ_RM_UNROLL
        for (int j = i; j < 3; ++j) {
            const int u = i == 0 ? j : (i == 1 ? 2 + j : 5);
            double q0[10], q1[10], q2[10];
            akz_fp_o1(AKZ_FP_EP(i, 0), AKZ_FP_EP(j, 0), q0);
            akz_fp_o1(AKZ_FP_EP(i, 1), AKZ_FP_EP(j, 1), q1);
            akz_fp_o1(AKZ_FP_EP(i, 2), AKZ_FP_EP(j, 2), q2);
            AKZ_RM_UNROLL
            for (int k = 0; k < 10; ++k) L[u][k] = (q0[k] + q1[k]) + q2[k];
        }
    }
    /* L = E E^T - 0.5 trace (lib.rs:186-191) */
    {
        double tr[10];
        AKZ_RM_UNROLL
        for (int k = 0; k < 10; ++k) tr[k] = 0.5 * ((L[0][k] + L[3][k]) + L[5][k]);
        AKZ_RM_UNROLL
        for (int k = 0; k < 10; ++k) {
            L[0][k] = L[0][k] - tr[k];
            L[3][k] = L[3][k] - tr[k];
            L[5][k] = L[5][k] - tr[k];
        }
    }
    /* rows 1 + 3 i + j = (L E)(i, j) (lib.rs:195-201) */
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        AKZ_RM_UNROLL
        for (int j = 0; j < 3; ++j) {
            /* l[i][k], k = 0, 1, 2 of the symmetric L */
            const int u0 = i == 0 ? 0 : (i == 1 ? 1 : 2);
            const int u1 = i == 0 ? 1 : (i == 1 ? 3 : 4);
            const int u2 = i == 0 ? 2 : (i == 1 ? 4 : 5);
            double t0[20], t1[20], t2[20];
            akz_fp_o2(L[u0], AKZ_FP_EP(0, j), t0);
            akz_fp_o2(L[u1], AKZ_FP_EP(1, j), t1);
            akz_fp_o2(L[u2], AKZ_FP_EP(2, j), t2);
            AKZ_RM_UNROLL
            for (int k = 0; k < 20; ++k) w[((1 + 3 * i + j) * 20 + k) * S] = (t0[k] + t1[k]) + t2[k];
        }
    }
#undef AKZ_FP_EP
}

#define AKZ_FP_M(r, c) w[((r) * 20 + (c)) * S]

/* ---- step 3: Gauss-Jordan elimination of the left 10 x 10 block against the right one (lib.rs:256-261), partial
 * pivoting.  Afterwards columns 10..19 hold the solution X of C_left X = C_right.  Returns 0 on a zero or non-finite
 * pivot. */
AKZ_RM_FN int akz_fp_eliminate(double* w, int S)
{
    for (int k = 0; k < 10; ++k) {
        int pr = k;
        double best = AKZ_FP_ABS(AKZ_FP_M(k, k));
        for (int r = k + 1; r < 10; ++r) {
            const double v = AKZ_FP_ABS(AKZ_FP_M(r, k));
            if (v > best) {
                best = v;
                pr = r;
            }
        }
        if (!(best > 0.0) || !AKZ_FP_FINITE(best)) return 0;
        if (pr != k)
            for (int c = k; c < 20; ++c) {
                const double t = AKZ_FP_M(k, c);
                AKZ_FP_M(k, c) = AKZ_FP_M(pr, c);
                AKZ_FP_M(pr, c) = t;
            }
        const double piv = AKZ_FP_M(k, k);
        for (int c = k; c < 20; ++c) AKZ_FP_M(k, c) = AKZ_FP_M(k, c) / piv;
        for (int r = 0; r < 10; ++r) {
            if (r == k) continue;
            const double f = AKZ_FP_M(r, k);
            if (f == 0.0) continue;
            for (int c = k; c < 20; ++c) AKZ_FP_M(r, c) = AKZ_FP_M(r, c) - f * AKZ_FP_M(k, c);
        }
    }
    return 1;
}

/* ---- step 4: the action matrix (lib.rs:267-277), entry (r, c), read out of the eliminated matrix */
AKZ_RM_FN double akz_fp_action(const double* w, int S, int r, int c)
{
    if (r < 6) {
        const int src = r < 3 ? r : (r == 3 ? 4 : (r == 4 ? 5 : 7));
        return AKZ_FP_M(src, 10 + c);
    }
    const int one = r == 6 ? 0 : (r == 7 ? 1 : (r == 8 ? 3 : 6));
    return c == one ? -1.0 : 0.0;
}

/* the 10 x 10 work matrix lives in columns 0..9 of the eliminated matrix (an identity nobody needs any more) */
#define AKZ_FP_H(r, c) w[((r) * 20 + (c)) * S]
#define AKZ_FP_WR(i) w[(200 + (i)) * S]
#define AKZ_FP_WI(i) w[(210 + (i)) * S]
#define AKZ_FP_PERM(i) w[(220 + (i)) * S]
#define AKZ_FP_VEC(i) w[(230 + (i)) * S]

AKZ_RM_FN double akz_fp_sign(double a, double b) { const double m = AKZ_FP_ABS(a); return b >= 0.0 ? m : -m; }

/* ---- step 5: all eigenvalues of the action matrix -> AKZ_FP_WR / AKZ_FP_WI.  Returns 0 when an eigenvalue needed more
 * than AKZ_FP_QR_ITERS iterations. */
AKZ_RM_FN int akz_fp_eigenvalues(double* w, int S)
{
    const int n = 10;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) AKZ_FP_H(r, c) = akz_fp_action(w, S, r, c);
    /* Hessenberg form by stabilised elementary similarity transformations */
    for (int m = 1; m < n - 1; ++m) {
        double x = 0.0;
        int i = m;
        for (int j = m; j < n; ++j) {
            const double v = AKZ_FP_H(j, m - 1);
            if (AKZ_FP_ABS(v) > AKZ_FP_ABS(x)) {
                x = v;
                i = j;
            }
        }
        if (i != m) {
            for (int j = m - 1; j < n; ++j) {
                const double t = AKZ_FP_H(i, j);
                AKZ_FP_H(i, j) = AKZ_FP_H(m, j);
                AKZ_FP_H(m, j) = t;
            }
            for (int j = 0; j < n; ++j) {
                const double t = AKZ_FP_H(j, i);
                AKZ_FP_H(j, i) = AKZ_FP_H(j, m);
                AKZ_FP_H(j, m) = t;
            }
        }
        if (x != 0.0) {
            for (int r = m + 1; r < n; ++r) {
                double y = AKZ_FP_H(r, m - 1);
                if (y != 0.0) {
                    y = y / x;
                    for (int j = m; j < n; ++j) AKZ_FP_H(r, j) = AKZ_FP_H(r, j) - y * AKZ_FP_H(m, j);
                    for (int j = 0; j < n; ++j) AKZ_FP_H(j, m) = AKZ_FP_H(j, m) + y * AKZ_FP_H(j, r);
                }
            }
        }
    }
    for (int r = 2; r < n; ++r)
        for (int c = 0; c < r - 1; ++c) AKZ_FP_H(r, c) = 0.0;
    /* Francis double-shift QR on the Hessenberg matrix */
    double anorm = 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = (r > 0 ? r - 1 : 0); c < n; ++c) anorm = anorm + AKZ_FP_ABS(AKZ_FP_H(r, c));
    int nn = n - 1;
    double t = 0.0;
    double p = 0.0, q = 0.0, r = 0.0, s = 0.0, x = 0.0, y = 0.0, z = 0.0, ww = 0.0;
    while (nn >= 0) {
        int its = 0, l;
        do {
            for (l = nn; l >= 1; --l) {
                s = AKZ_FP_ABS(AKZ_FP_H(l - 1, l - 1)) + AKZ_FP_ABS(AKZ_FP_H(l, l));
                if (s == 0.0) s = anorm;
                if (AKZ_FP_ABS(AKZ_FP_H(l, l - 1)) + s == s) {
                    AKZ_FP_H(l, l - 1) = 0.0;
                    break;
                }
            }
            x = AKZ_FP_H(nn, nn);
            if (l == nn) { /* one root */
                AKZ_FP_WR(nn) = x + t;
                AKZ_FP_WI(nn) = 0.0;
                nn = nn - 1;
            } else {
                y = AKZ_FP_H(nn - 1, nn - 1);
                ww = AKZ_FP_H(nn, nn - 1) * AKZ_FP_H(nn - 1, nn);
                if (l == nn - 1) { /* two roots */
                    p = 0.5 * (y - x);
                    q = p * p + ww;
                    z = AKZ_RM_SQRT(AKZ_FP_ABS(q));
                    x = x + t;
                    if (q >= 0.0) {
                        z = p + akz_fp_sign(z, p);
                        AKZ_FP_WR(nn - 1) = x + z;
                        AKZ_FP_WR(nn) = x + z;
                        if (z != 0.0) AKZ_FP_WR(nn) = x - ww / z;
                        AKZ_FP_WI(nn - 1) = 0.0;
                        AKZ_FP_WI(nn) = 0.0;
                    } else {
                        AKZ_FP_WR(nn - 1) = x + p;
                        AKZ_FP_WR(nn) = x + p;
                        AKZ_FP_WI(nn - 1) = -z;
                        AKZ_FP_WI(nn) = z;
                    }
                    nn = nn - 2;
                } else {
                    if (its >= AKZ_FP_QR_ITERS) return 0;
                    if (its == 10 || its == 20) { /* exceptional shift */
                        t = t + x;
                        for (int i = 0; i <= nn; ++i) AKZ_FP_H(i, i) = AKZ_FP_H(i, i) - x;
                        s = AKZ_FP_ABS(AKZ_FP_H(nn, nn - 1)) + AKZ_FP_ABS(AKZ_FP_H(nn - 1, nn - 2));
                        x = 0.75 * s;
                        y = x;
                        ww = -0.4375 * s * s;
                    }
                    ++its;
                    int m;
                    for (m = nn - 2; m >= l; --m) {
                        z = AKZ_FP_H(m, m);
                        r = x - z;
                        s = y - z;
                        p = (r * s - ww) / AKZ_FP_H(m + 1, m) + AKZ_FP_H(m, m + 1);
                        q = AKZ_FP_H(m + 1, m + 1) - z - r - s;
                        r = AKZ_FP_H(m + 2, m + 1);
                        s = AKZ_FP_ABS(p) + AKZ_FP_ABS(q) + AKZ_FP_ABS(r);
                        p = p / s;
                        q = q / s;
                        r = r / s;
                        if (m == l) break;
                        const double u = AKZ_FP_ABS(AKZ_FP_H(m, m - 1)) * (AKZ_FP_ABS(q) + AKZ_FP_ABS(r));
                        const double v = AKZ_FP_ABS(p) * (AKZ_FP_ABS(AKZ_FP_H(m - 1, m - 1)) + AKZ_FP_ABS(z) + AKZ_FP_ABS(AKZ_FP_H(m + 1, m + 1)));
                        if (u + v == v) break;
                    }
                    for (int i = m + 2; i <= nn; ++i) {
                        AKZ_FP_H(i, i - 2) = 0.0;
                        if (i != m + 2) AKZ_FP_H(i, i - 3) = 0.0;
                    }
                    for (int k = m; k <= nn - 1; ++k) {
                        if (k != m) {
                            p = AKZ_FP_H(k, k - 1);
                            q = AKZ_FP_H(k + 1, k - 1);
                            r = 0.0;
                            if (k != nn - 1) r = AKZ_FP_H(k + 2, k - 1);
                            x = AKZ_FP_ABS(p) + AKZ_FP_ABS(q) + AKZ_FP_ABS(r);
                            if (x != 0.0) {
                                p = p / x;
                                q = q / x;
                                r = r / x;
                            }
                        }
                        s = akz_fp_sign(AKZ_RM_SQRT(p * p + q * q + r * r), p);
                        if (s != 0.0) {
                            if (k == m) {
                                if (l != m) AKZ_FP_H(k, k - 1) = -AKZ_FP_H(k, k - 1);
                            } else
                                AKZ_FP_H(k, k - 1) = -s * x;
                            p = p + s;
                            x = p / s;
                            y = q / s;
                            z = r / s;
                            q = q / p;
                            r = r / p;
                            for (int j = k; j <= nn; ++j) {
                                p = AKZ_FP_H(k, j) + q * AKZ_FP_H(k + 1, j);
                                if (k != nn - 1) {
                                    p = p + r * AKZ_FP_H(k + 2, j);
                                    AKZ_FP_H(k + 2, j) = AKZ_FP_H(k + 2, j) - p * z;
                                }
                                AKZ_FP_H(k + 1, j) = AKZ_FP_H(k + 1, j) - p * y;
                                AKZ_FP_H(k, j) = AKZ_FP_H(k, j) - p * x;
                            }
                            const int mmin = nn < k + 3 ? nn : k + 3;
                            for (int i = l; i <= mmin; ++i) {
                                p = x * AKZ_FP_H(i, k) + y * AKZ_FP_H(i, k + 1);
                                if (k != nn - 1) {
                                    p = p + z * AKZ_FP_H(i, k + 2);
                                    AKZ_FP_H(i, k + 2) = AKZ_FP_H(i, k + 2) - p * r;
                                }
                                AKZ_FP_H(i, k + 1) = AKZ_FP_H(i, k + 1) - p * q;
                                AKZ_FP_H(i, k) = AKZ_FP_H(i, k) - p;
                            }
                        }
                    }
                }
            }
        } while (l < nn - 1);
    }
    return 1;
}

/* ---- step 6: the null vector of At - lambda I -> AKZ_FP_VEC, unit length.  Returns 0 when it is not finite. */
AKZ_RM_FN int akz_fp_eigenvector(double* w, int S, double lambda)
{
    const int n = 10;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            const double v = akz_fp_action(w, S, r, c);
            AKZ_FP_H(r, c) = r == c ? v - lambda : v;
        }
    for (int i = 0; i < n; ++i) AKZ_FP_PERM(i) = (double)i;
    for (int k = 0; k < n - 1; ++k) {
        int pr = k, pc = k;
        double best = -1.0;
        for (int r = k; r < n; ++r)
            for (int c = k; c < n; ++c) {
                const double v = AKZ_FP_ABS(AKZ_FP_H(r, c));
                if (v > best) {
                    best = v;
                    pr = r;
                    pc = c;
                }
            }
        if (!(best > 0.0)) break; /* the rest is exactly zero (or not a number): back substitution below sees zeros */
        if (pr != k)
            for (int c = 0; c < n; ++c) {
                const double tv = AKZ_FP_H(k, c);
                AKZ_FP_H(k, c) = AKZ_FP_H(pr, c);
                AKZ_FP_H(pr, c) = tv;
            }
        if (pc != k) {
            for (int r = 0; r < n; ++r) {
                const double tv = AKZ_FP_H(r, k);
                AKZ_FP_H(r, k) = AKZ_FP_H(r, pc);
                AKZ_FP_H(r, pc) = tv;
            }
            const double tp = AKZ_FP_PERM(k);
            AKZ_FP_PERM(k) = AKZ_FP_PERM(pc);
            AKZ_FP_PERM(pc) = tp;
        }
        const double piv = AKZ_FP_H(k, k);
        for (int r = k + 1; r < n; ++r) {
            const double f = AKZ_FP_H(r, k) / piv;
            if (f == 0.0) continue;
            for (int c = k + 1; c < n; ++c) AKZ_FP_H(r, c) = AKZ_FP_H(r, c) - f * AKZ_FP_H(k, c);
        }
    }
    /* U z = 0 with z[9] = 1 (the last pivot is taken as zero): z[k] = -(sum_{c > k} U(k, c) z[c]) / U(k, k), k = 8 .. 0.
     * z sits in AKZ_FP_WI's place: the imaginary parts are no longer needed once the real eigenvalues are packed. */
#define AKZ_FP_Z(i) w[(210 + (i)) * S]
    AKZ_FP_Z(9) = 1.0;
    double norm2 = 1.0;
    for (int k = n - 2; k >= 0; --k) {
        double acc = 0.0;
        for (int c = k + 1; c < n; ++c) acc = acc + AKZ_FP_H(k, c) * AKZ_FP_Z(c);
        const double zk = -acc / AKZ_FP_H(k, k);
        AKZ_FP_Z(k) = zk;
        norm2 = norm2 + zk * zk;
    }
    const double nrm = AKZ_RM_SQRT(norm2);
    int fin = AKZ_FP_FINITE(nrm);
    for (int k = 0; k < n; ++k) {
        const double zk = AKZ_FP_Z(k) / nrm;
        fin = fin && AKZ_FP_FINITE(zk);
        AKZ_FP_VEC((int)AKZ_FP_PERM(k)) = zk;
    }
#undef AKZ_FP_Z
    return fin;
}

/* ---- steps 2-6 for one sample whose null space is known.  basis: 9 x 4 (akz_fp_nullspace); w: AKZ_FP_WORK doubles at
 * stride S; E_out: element (solution s, entry e) at E_out[(s * 9 + e) * ES], E row-major with b^T E a = 0 (the reference's
 * Matrix3::from_iterator over basis * (x, y, z, 1) is column-major).  Returns the number of solutions, 0..10, in ascending
 * order of eigenvalue; slots beyond it are not written. */
AKZ_RM_FN int akz_fp_solve(const double* basis, double* w, int S, double* E_out, int ES)
{
    akz_fp_constraints(basis, w, S);
    if (!akz_fp_eliminate(w, S)) return 0;
    if (!akz_fp_eigenvalues(w, S)) return 0;
    /* the real eigenvalues, ascending (stable insertion sort), packed at AKZ_FP_WR(0 .. n_real - 1) */
    int n_real = 0;
    for (int i = 0; i < 10; ++i) {
        if (AKZ_FP_WI(i) != 0.0) continue;
        const double v = AKZ_FP_WR(i);
        if (!AKZ_FP_FINITE(v)) continue;
        int at = n_real;
        while (at > 0 && AKZ_FP_WR(at - 1) > v) {
            AKZ_FP_WR(at) = AKZ_FP_WR(at - 1);
            --at;
        }
        AKZ_FP_WR(at) = v;
        ++n_real;
    }
    int n_sol = 0;
    for (int i = 0; i < n_real; ++i) {
        if (!akz_fp_eigenvector(w, S, AKZ_FP_WR(i))) continue;
        const double x = AKZ_FP_VEC(6), y = AKZ_FP_VEC(7), z = AKZ_FP_VEC(8), o = AKZ_FP_VEC(9);
        double e[9];
        int fin = 1;
        AKZ_RM_UNROLL
        for (int k = 0; k < 9; ++k) {
            e[k] = ((basis[k * 4 + 0] * x + basis[k * 4 + 1] * y) + basis[k * 4 + 2] * z) + basis[k * 4 + 3] * o;
            fin = fin && AKZ_FP_FINITE(e[k]);
        }
        if (!fin) continue;
        AKZ_RM_UNROLL
        for (int r = 0; r < 3; ++r) {
            AKZ_RM_UNROLL
            for (int c = 0; c < 3; ++c) E_out[((n_sol * 9) + r * 3 + c) * ES] = e[c * 3 + r];
        }
        ++n_sol;
    }
    return n_sol;
}

/* the whole solver for one sample (host form: S = 1).  E_out[10][9]. */
AKZ_RM_FN int akz_five_point_essentials(const double* a5, const double* b5, double eps, int max_sweeps, double* E_out)
{
    double basis[36], w[AKZ_FP_WORK];
    if (!akz_fp_nullspace(a5, b5, eps, max_sweeps, basis)) return 0;
    return akz_fp_solve(basis, w, 1, E_out, 1);
}

#endif /* AKZ_FIVE_POINT_MATH_H */
