// Host build of the launch shape of the per-read counters (minorseq_amd/csrc/readstats_shape.h) so that it can be checked, and its
// edges named, without a GPU (tests/test_readstats_host.py, tests/test_gpu_readstats.py).  Not part of the product.
#include "../../minorseq_amd/csrc/readstats_shape.h"
// out[0..6] = wg_reads, n_chunks, seg_cols, n_segs, k, flush, combine
extern "C" void shim_readstats_shape(uint64_t n_reads, uint32_t n_cols, uint32_t *out)
{
    const jl_readstats_shape s = jl_readstats_shape_for(n_reads, n_cols);
    out[0] = s.wg_reads, out[1] = s.n_chunks, out[2] = s.seg_cols, out[3] = s.n_segs, out[4] = s.k, out[5] = s.flush, out[6] = s.combine;
}
