// Host build of the launch shape of the per-read reading-frame counters (minorseq_amd/csrc/orf_shape.h) so that it can be checked,
// and its edges named, without a GPU (tests/test_orf_host.py, tests/test_gpu_orf.py).  Not part of the product.
#include "../../minorseq_amd/csrc/orf_shape.h"
// out[0..6] = wg_reads, n_chunks, seg_codons, k, flush_codons, n_segs, grid (cut to 32 bits); span_segs[n_spans]
// k == 0: the library's own slice count
extern "C" void shim_orf_shape(const uint32_t *n_codons, uint32_t n_spans, uint64_t n_reads, uint32_t k, uint32_t *out, uint32_t *span_segs)
{
    const jl_orf_shape s = jl_orf_shape_for(n_codons, n_spans, n_reads, k ? k : JL_ORF_K);
    out[0] = s.wg_reads, out[1] = s.n_chunks, out[2] = s.seg_codons, out[3] = s.k, out[4] = s.flush_codons, out[5] = s.n_segs;
    out[6] = (uint32_t)s.grid;
    for (uint32_t g = 0; g < n_spans; ++g) span_segs[g] = s.span_segs[g];
}
// out[0..3] = JL_ORF_SHAPE_MAX_SPANS, JL_ORF_SEG_CODONS_MAX, JL_ORF_SEG_CODONS_MIN, JL_ORF_K
extern "C" void shim_orf_constants(uint32_t *out)
{
    out[0] = JL_ORF_SHAPE_MAX_SPANS, out[1] = JL_ORF_SEG_CODONS_MAX, out[2] = JL_ORF_SEG_CODONS_MIN, out[3] = JL_ORF_K;
}
