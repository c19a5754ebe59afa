// Host build of the pure helpers of the plane-row tile walk (minorseq_amd/csrc/planes.h, the host half of plane_walk.h) so that
// they can be checked without a GPU (tests/test_walk_host.py).  Not part of the product.
#include "../../minorseq_amd/csrc/plane_walk.h"
extern "C" uint32_t shim_valid_bits(uint64_t n_reads, uint64_t word)
{
    return jl_valid_bits(n_reads, word);
}
extern "C" uint32_t shim_walk_tiles(uint64_t n_reads)
{
    return jl_walk_tiles(n_reads);
}
extern "C" void shim_walk_shape(uint64_t n_reads, uint32_t n_groups, uint32_t *seg_tiles, uint32_t *n_segs)
{
    const jl_walk_shape s = jl_walk_shape_for(n_reads, n_groups);
    *seg_tiles = s.seg_tiles, *n_segs = s.n_segs;
}
extern "C" void shim_class_codons_shape(uint64_t n_reads, uint32_t n_pos, uint32_t n_classes, uint32_t *seg_tiles, uint32_t *n_segs)
{
    const jl_walk_shape s = jl_class_codons_shape_for(n_reads, n_pos, n_classes);
    *seg_tiles = s.seg_tiles, *n_segs = s.n_segs;
}
