/* The CPU checker of the five-point kernels: thin exported wrappers around include/akz_five_point_math.h, the text
 * cv_amd/csrc/rs_ransac.hip compiles for the device.  tests/five_point_checker.py has tests/host_build.py build this with
 * the host compiler (its `load`: -O2, no contraction to FMA) into a shared object and loads it with ctypes. */
#include <stddef.h>
#include <stdint.h>

#include "../../include/akz_five_point_math.h"

/* bearings a / b [n][3], samples [n_samples][5] -> E [n_samples][10][9] (slots beyond a sample's count are left as they
 * are), n_solutions [n_samples] */
void fp_essentials(const double* a, const double* b, const uint32_t* samples, uint32_t n_samples, double eps, int max_sweeps,
                   double* E, uint32_t* n_solutions)
{
    for (uint32_t s = 0; s < n_samples; ++s) {
        double a5[15], b5[15];
        for (int i = 0; i < 5; ++i)
            for (int k = 0; k < 3; ++k) {
                a5[3 * i + k] = a[(size_t)3 * samples[5 * s + i] + k];
                b5[3 * i + k] = b[(size_t)3 * samples[5 * s + i] + k];
            }
        n_solutions[s] = (uint32_t)akz_five_point_essentials(a5, b5, eps, max_sweeps, E + (size_t)90 * s);
    }
}

int fp_nullspace(const double* a5, const double* b5, double eps, int max_sweeps, double* basis)
{
    return akz_fp_nullspace(a5, b5, eps, max_sweeps, basis);
}

/* o1 of two linear forms -> the twenty entries of the reference's PolyBasisVec */
void fp_o1(const double* a, const double* b, double* out20)
{
    for (int k = 0; k < 10; ++k) out20[k] = 0.0;
    akz_fp_o1(a, b, out20 + 10);
}

/* o2 of a quadratic (its entries 10..19) and a linear form */
void fp_o2(const double* a20, const double* b, double* out20) { akz_fp_o2(a20 + 10, b, out20); }
