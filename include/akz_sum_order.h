/* akz_sum_order.h — THE ORDER OF A SUM OVER ITEMS that a wavefront or a workgroup forms, stated once.  The reference adds its
 * items (landmarks' gradients, a view's edges) one after another; a wavefront cannot.  Floating-point addition does not
 * associate, so "host build == HIP, bit for bit" needs one order on both sides.  It is, for waves of AKZ_SUM_WAVE = 64 lanes:
 *
 *   1. thread t of T holds ((0 + q[t]) + q[t + T]) + q[t + 2 T] ..., its items ascending; a thread without an item, and an
 *      item that contributes nothing, leave +0.0.  What an item's term q is, and T, is the caller's: T = 64 for the stages
 *      that give a wave its own sum (akz_three_view_constraint_math.h, akz_pose_graph_math.h), T = AKZ_SUM_THREADS = 256 for
 *      those that give one to a workgroup (akz_three_view_math.h, akz_single_view_math.h);
 *   2. inside a wave the butterfly v[l] = v[l] + v[l ^ m] for m = 32, 16, 8, 4, 2, 1.  IEEE addition commutes (a + b and
 *      b + a are the same bits), so both lanes of a pair, and in the end all 64 lanes, hold the same bits;
 *   3. for a workgroup, the waves' sums folded from the left in wave order: ((w0 + w1) + w2) + w3.
 *
 * The functions below execute steps 2 and 3 for the host builds.  On the device they are akz_wave_sum and akz_block_sum of
 * cv_amd/csrc/akz_common.h.  tests/test_sum_order.py states the same order in numpy and holds the host builds to it.
 */
#ifndef AKZ_SUM_ORDER_H
#define AKZ_SUM_ORDER_H

enum { AKZ_SUM_WAVE = 64, AKZ_SUM_THREADS = 256 };

/* step 2 over the 64 lanes' values v[0], v[stride], ..., v[63 * stride]: what lane 0 (and every lane) ends with */
static inline double akz_sum_wave(const double* v, unsigned stride)
{
    double tmp[AKZ_SUM_WAVE], nxt[AKZ_SUM_WAVE];
    for (int l = 0; l < AKZ_SUM_WAVE; ++l) tmp[l] = v[(unsigned)l * stride];
    for (int m = AKZ_SUM_WAVE / 2; m >= 1; m >>= 1) {
        for (int l = 0; l < AKZ_SUM_WAVE; ++l) nxt[l] = tmp[l] + tmp[l ^ m];
        for (int l = 0; l < AKZ_SUM_WAVE; ++l) tmp[l] = nxt[l];
    }
    return tmp[0];
}

/* steps 2 and 3 over the 256 threads' partial sums part[t * k + j] of k components: net[j] */
static inline void akz_sum_block(const double* part, unsigned k, double* net)
{
    for (unsigned j = 0; j < k; ++j) {
        double s = akz_sum_wave(part + j, k);
        for (unsigned w = 1; w < (unsigned)(AKZ_SUM_THREADS / AKZ_SUM_WAVE); ++w) s = s + akz_sum_wave(part + w * AKZ_SUM_WAVE * k + j, k);
        net[j] = s;
    }
}

#endif
