// readstats_shape.h — the launch shape of the per-read counters (kernels_readstats.hip, jl_read_stats_async; docs/SPEC.md §20), as
// jl_walk_shape_for is that of the column counters: one host-visible function, so that the tests can name its edges
// (tests/csrc/readstats_shape_shim.cpp).  Private to libjuliet_hip.so.
// A workgroup is one wave.  Lane l owns ONE 32-read word of every plane row — word 64 chunk + l, 2048 reads a workgroup — and
// walks the columns of its SEGMENT.  Per column a one-bit-per-read mask is added into each of five bit-sliced counters of k
// words; after flush = 2^k - 1 columns the slices are emptied into byte counters (four reads a dword, in LDS), which is why a
// segment holds at most 255 columns.  The bytes of all segments are summed exactly: by a second kernel over the segments' stored
// bytes (JL_RS_COMBINE_KERNEL), or by integer atomics into the zeroed output (JL_RS_COMBINE_ATOMIC).
#pragma once
#include <stdint.h>

#include <algorithm>

enum { JL_RS_COMBINE_KERNEL = 0, JL_RS_COMBINE_ATOMIC = 1 };

constexpr uint32_t JL_RS_WG_READS = 2048;      // reads of a workgroup: 64 lanes x one word
constexpr uint32_t JL_RS_SEG_COLS_MAX = 255;   // what a byte counter holds
constexpr uint32_t JL_RS_SEG_COLS_MIN = 64;    // a segment shorter than this (of a longer window) pays more for its epilogue than for its columns

struct jl_readstats_shape {
    uint32_t wg_reads;    // JL_RS_WG_READS
    uint32_t n_chunks;    // workgroups along the reads: ceil(n_reads / wg_reads)
    uint32_t seg_cols;    // columns of a segment: 1 .. JL_RS_SEG_COLS_MAX
    uint32_t n_segs;      // ceil(n_cols / seg_cols); the grid is n_chunks * n_segs workgroups
    uint32_t k;           // slices of a counter
    uint32_t flush;       // 2^k - 1: columns between two flushes
    uint32_t combine;     // JL_RS_COMBINE_*
};

// n_reads > 0, n_cols > 0.  Segments x chunks fill the chip about twice (sixteen workgroups fit a CU by their LDS), as long as a
// segment keeps JL_RS_SEG_COLS_MIN columns: every segment costs 5 bytes per read to combine.
// k and the combine form are the fastest of those measured on the bench window ("Per-read counters").
static inline jl_readstats_shape jl_readstats_shape_for(uint64_t n_reads, uint32_t n_cols)
{
    const uint32_t want_blocks = 2048u;
    jl_readstats_shape s;
    s.wg_reads = JL_RS_WG_READS;
    s.n_chunks = (uint32_t)((n_reads + JL_RS_WG_READS - 1u) / JL_RS_WG_READS);
    const uint32_t segs = std::max(1u, want_blocks / std::max(1u, s.n_chunks));
    const uint32_t even = (uint32_t)(((uint64_t)n_cols + segs - 1u) / segs);
    s.seg_cols = std::min(std::min(JL_RS_SEG_COLS_MAX, n_cols), std::max(JL_RS_SEG_COLS_MIN, even));
    s.n_segs = (n_cols + s.seg_cols - 1u) / s.seg_cols;
    s.k = 4u;
    s.flush = (1u << s.k) - 1u;
    s.combine = JL_RS_COMBINE_KERNEL;
    return s;
}
