// Host build of minorseq_amd/csrc/jl_fisher.h so the algorithm the device runs can be checked against
// the mpmath golden vectors without a GPU (tests/test_fisher_host.py).  Not part of the product.
#include "../../minorseq_amd/csrc/jl_fisher.h"
extern "C" double shim_fisher(uint32_t a, uint32_t c, uint32_t n, double *lp)
{
    return jl_fisher_greater_equal_rows(a, c, n, lp);
}
extern "C" double shim_fisher_two_sided(uint32_t a, uint32_t c, uint32_t n, double *lp)
{
    return jl_fisher_two_sided_equal_rows(a, c, n, lp);
}
// the form call_eval.h calls: *skipped = 1 where the tail sum was not needed (the point mass alone rules a call out)
extern "C" double shim_fisher_or_skip(uint32_t a, uint32_t c, uint32_t n, double n_tests, double alpha, double *lp, int *skipped)
{
    bool s;
    const double p = jl_fisher_greater_equal_rows_or_skip(a, c, n, n_tests, alpha, lp, &s);
    *skipped = s ? 1 : 0;
    return p;
}
