// orf_shape.h — the launch shape of the per-read reading-frame counters (kernels_orf.hip, jl_read_orf_async; docs/SPEC.md §27), as
// jl_readstats_shape_for is that of the per-read counters: one host-visible function, so that the tests can name its edges
// (tests/csrc/orf_shape_shim.cpp).  Private to libjuliet_hip.so.
// A workgroup is one wave.  Lane l owns ONE 32-read word of every plane row — word 64 chunk + l, 2048 reads a workgroup — and
// walks ONE SEGMENT of ONE span: whole codons of that span, seg_codons of them but for the span's last segment, which holds the
// rest.  Segment s of a span begins at its codon s * seg_codons, so the segments tile every span exactly, none crosses a span, and
// none needs a column outside its own (no halo).  Per column a one-bit-per-read mask goes into bit-sliced counters of k words;
// COVERED and GAP_CELLS take three additions a codon, so the slices are emptied into byte counters after flush_codons =
// floor((2^k - 1) / 3) codons, and a segment holds at most 85 codons: 255 columns, what a byte counter holds.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "readstats_shape.h"

constexpr uint32_t JL_ORF_SHAPE_MAX_SPANS = 64;     // JL_ORF_MAX_SPANS of include/juliet_hip.h
constexpr uint32_t JL_ORF_SEG_CODONS_MAX = 85;      // 255 columns: what a byte counter holds
constexpr uint32_t JL_ORF_SEG_CODONS_MIN = 22;      // as JL_RS_SEG_COLS_MIN: a shorter segment (of a longer span) pays more for its epilogue than for its columns
constexpr uint32_t JL_ORF_K = 4;                    // slices of a counter: the per-read counters' (readstats_shape.h)

struct jl_orf_shape {
    uint32_t wg_reads;        // JL_RS_WG_READS
    uint32_t n_chunks;        // workgroups along the reads: ceil(n_reads / wg_reads)
    uint32_t seg_codons;      // codons of a segment: 1 .. JL_ORF_SEG_CODONS_MAX
    uint32_t k;               // slices of a counter
    uint32_t flush_codons;    // floor((2^k - 1) / 3): codons between two flushes
    uint32_t n_segs;          // segments of all spans; the grid is n_chunks * n_segs workgroups (64 bits: grid)
    uint64_t grid;
    uint32_t span_segs[JL_ORF_SHAPE_MAX_SPANS];   // segments of span g: ceil(n_codons[g] / seg_codons)
};

// n_reads > 0; 1 <= n_spans <= 64; every n_codons[g] >= 1 (and 3 n_codons[g] <= n_cols <= 2^32 - 1: the sums fit); k in 4 .. 6.
// Segments x chunks fill the chip about twice, as the per-read counters' do, as long as a segment keeps JL_ORF_SEG_CODONS_MIN
// codons: every segment costs 5 bytes per read to combine.
static inline jl_orf_shape jl_orf_shape_for(const uint32_t *n_codons, uint32_t n_spans, uint64_t n_reads, uint32_t k)
{
    const uint32_t want_blocks = 2048u;
    jl_orf_shape s = {};
    s.wg_reads = JL_RS_WG_READS;
    s.n_chunks = (uint32_t)((n_reads + JL_RS_WG_READS - 1u) / JL_RS_WG_READS);
    uint64_t total = 0;
    for (uint32_t g = 0; g < n_spans; ++g) total += n_codons[g];
    const uint64_t segs = std::max(1u, want_blocks / std::max(1u, s.n_chunks));
    const uint64_t even = (total + segs - 1u) / segs;
    s.seg_codons = (uint32_t)std::min<uint64_t>(JL_ORF_SEG_CODONS_MAX, std::max<uint64_t>(JL_ORF_SEG_CODONS_MIN, even));
    s.k = k;
    s.flush_codons = ((1u << k) - 1u) / 3u;
    uint64_t n_segs = 0;
    for (uint32_t g = 0; g < n_spans; ++g) {
        s.span_segs[g] = (n_codons[g] + s.seg_codons - 1u) / s.seg_codons;
        n_segs += s.span_segs[g];
    }
    s.n_segs = (uint32_t)std::min<uint64_t>(n_segs, 0xFFFFFFFFull);
    s.grid = n_segs * s.n_chunks;
    return s;
}
