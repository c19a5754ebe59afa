// deviation_index.h — the deviation index of a resident window: format and bounds (host and device; DESIGN.md "The deviation index").
// Per plain codon chunk (three own columns, a codon start at the first, no halo) a list of the reads whose code differs from the
// chunk's INDEX SEED — the exact majority base among A C G T of each column, a property of the cells alone — in at least one of
// the three columns.  A read that is not in the list carries the seed base in all three columns: the counting kernel
// (kernels_pileup.hip pileup_index_body) adds n_reads - E to the seed's bins and walks E entries instead of nine plane rows.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JL_IX_FN __host__ __device__ __forceinline__
#else
#define JL_IX_FN static inline
#endif

// ---- the entry: read number in the upper 23 bits, the three 3-bit codes (columns c0, c0 + 1, c0 + 2) in the lower nine
#define JL_IX_READ_BITS 23u
#define JL_IX_MAX_READS (1ull << JL_IX_READ_BITS)   // windows with more reads get no index
JL_IX_FN uint32_t jl_ix_encode(uint32_t read, uint32_t a, uint32_t b, uint32_t c) { return (read << 9) | (a << 6) | (b << 3) | c; }
JL_IX_FN uint32_t jl_ix_read(uint32_t e) { return e >> 9; }
JL_IX_FN uint32_t jl_ix_code(uint32_t e, uint32_t j) { return (e >> (6u - 3u * j)) & 7u; }   // j = 0, 1, 2

// ---- bounds.  A chunk is indexed while its entries take at most half of its nine plane rows' bytes: below that the list wins
// whenever the entry walk sustains half of the plane kernel's byte rate.  The window has an index while all its lists together
// take at most half of the matrix's plane bytes.  (numerator / denominator: the sweep of profiles/ changes these two only)
#ifndef JL_IX_DENSITY_NUM
#define JL_IX_DENSITY_NUM 1u
#define JL_IX_DENSITY_DEN 2u
#endif
// most entries of an indexed chunk: 4 E <= 9 plane_stride NUM / DEN
JL_IX_FN uint64_t jl_ix_chunk_max_entries(uint64_t plane_stride) { return 9u * plane_stride * JL_IX_DENSITY_NUM / (4u * JL_IX_DENSITY_DEN); }
// a chunk's list begins on 16 bytes (a lane loads four entries at once): its room in the buffer
JL_IX_FN uint64_t jl_ix_padded(uint64_t entries) { return (entries + 3u) & ~(uint64_t)3u; }
// most entries (padded) of a whole index: half of the matrix's plane bytes.  While a chunk's bound is at most half of its own plane
// bytes the plain chunks' bounds add up to no more than this, so this bound only limits the allocation when the density bound
// (JL_IX_DENSITY_NUM / DEN) is swept above a half; an index is REFUSED in practice only when no chunk is under its own bound.
JL_IX_FN uint64_t jl_ix_total_max_entries(uint64_t plane_stride, uint32_t n_cols) { return 3u * (uint64_t)n_cols * plane_stride / 8u; }
// what is allocated before the build, with no host round trip in the middle: the smaller of the two bounds
JL_IX_FN uint64_t jl_ix_alloc_entries(uint64_t plane_stride, uint32_t n_cols, uint32_t n_plain)
{
    const uint64_t by_chunk = (uint64_t)n_plain * jl_ix_padded(jl_ix_chunk_max_entries(plane_stride));
    const uint64_t by_total = jl_ix_padded(jl_ix_total_max_entries(plane_stride, n_cols));
    return (by_chunk < by_total ? by_chunk : by_total) + 4u;
}

// ---- the counting kernel's per-lane accumulators: one 64-bit word per column, a 9-bit field per code 0..6 (63 bits).  A lane
// takes four entries a round (one 16-byte load), each adds one to one field of each column: a field holds at most 511, so a
// batch is at most 127 rounds (508), and the 64 lanes of a wave sum to at most 64 x 508 = 32512 < 2^16: two fields per DPP sum.
#define JL_IX_FIELD_BITS 9u
#define JL_IX_ROUND_ENTRIES 4u
#define JL_IX_FLUSH_ROUNDS 127u
#define JL_IX_BLOCK_LANES 256u
JL_IX_FN uint32_t jl_ix_field_max(void) { return (1u << JL_IX_FIELD_BITS) - 1u; }
// entries of a chunk that one workgroup walks without a flush in between: beyond it the flush edge is crossed
JL_IX_FN uint64_t jl_ix_flush_entries(void) { return (uint64_t)JL_IX_FLUSH_ROUNDS * JL_IX_ROUND_ENTRIES * JL_IX_BLOCK_LANES; }

// ---- the record a build leaves in pinned host memory (jl_ctx::h_ix) and jl_msa_index_info hands out
#define JL_IX_NONE 0u
#define JL_IX_PENDING 1u
#define JL_IX_BUILT 2u
#define JL_IX_REFUSED 3u
