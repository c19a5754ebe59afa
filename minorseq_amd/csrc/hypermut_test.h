// hypermut_test.h — the per-read test of docs/SPEC.md §26, written once for device (kernels_hypermut.hip) and host
// (jl_hypermut_test): P(X >= a) of the table [[a, n - a], [c, m - c]] of a read's target and control G->A counts by the
// general-margin routine of the control call; a read without target sites or without control sites is not tested.
#pragma once
#include "jl_fisher_general.h"

// a <= n target mutations of n target sites, c <= m control mutations of m control sites; returns p, *logp = ln p
JL_FHD double jl_hypermut_p(uint32_t a, uint32_t n, uint32_t c, uint32_t m, double *logp)
{
    if (n == 0u || m == 0u) {
        *logp = 0.0;
        return 1.0;
    }
    return jl_fisher_greater_general(a, n, c, m, logp);
}
