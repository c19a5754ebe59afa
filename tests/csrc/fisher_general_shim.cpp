// Host build of minorseq_amd/csrc/jl_fisher_general.h so the algorithm the device runs can be checked against the mpmath
// golden vectors without a GPU (tests/test_control_host.py).  Not part of the product.
#include "../../minorseq_amd/csrc/jl_fisher_general.h"
// the table [[a, n - a], [c, m - c]]
extern "C" double shim_fisher_general(uint32_t a, uint32_t n, uint32_t c, uint32_t m, double *lp)
{
    return jl_fisher_greater_general(a, n, c, m, lp);
}
// the form the kernel calls: *skipped = 1 where the tail sum was not needed (the point mass alone rules a call out)
extern "C" double shim_fisher_general_or_skip(uint32_t a, uint32_t n, uint32_t c, uint32_t m, double n_tests, double alpha, double *lp,
                                              int *skipped)
{
    bool s;
    const double p = jl_fisher_greater_general_or_skip(a, n, c, m, n_tests, alpha, lp, &s);
    *skipped = s ? 1 : 0;
    return p;
}
extern "C" double shim_fisher_equal_rows(uint32_t a, uint32_t c, uint32_t n, double *lp)
{
    return jl_fisher_greater_equal_rows(a, c, n, lp);
}
