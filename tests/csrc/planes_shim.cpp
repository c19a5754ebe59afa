// Host build of the bit helpers of the resident format (minorseq_amd/csrc/planes.h) so that they can be checked without a GPU
// (tests/test_planes_host.py), over arrays: one call per table.  Not part of the product.
#include "../../minorseq_amd/csrc/planes.h"
extern "C" void shim_plane_bits8(const uint32_t *w, uint32_t k, uint32_t *out, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = jl_plane_bits8(w[i], k);
}
extern "C" void shim_spread8(const uint32_t *b, uint32_t *out, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = jl_spread8(b[i]);
}
extern "C" void shim_planes_to_nibbles8(const uint32_t *b0, const uint32_t *b1, const uint32_t *b2, uint32_t *out, uint64_t n)
{
    for (uint64_t i = 0; i < n; ++i) out[i] = jl_planes_to_nibbles8(b0[i], b1[i], b2[i]);
}
