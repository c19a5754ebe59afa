// deviation_index.h — the deviation index of a resident window: format and bounds (host and device; DESIGN.md "The deviation index").
// Per plain codon chunk (three own columns, a codon start at the first, no halo) a list of the reads whose code differs from the
// chunk's INDEX SEED — the exact majority base among A C G T of each column, a property of the cells alone — in at least one of
// the three columns.  A read that is not in the list carries the seed base in all three columns: the counting kernel
// (kernels_pileup.hip pileup_index_body) adds n_reads - E to the seed's bins and walks E entries instead of nine plane rows.
// The STORED list carries the codes only, 16 bits an entry: counting asks what a deviating read carries, never which read it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JL_IX_FN __host__ __device__ __forceinline__
#else
#define JL_IX_FN static inline
#endif

// ---- the entry as the build forms it: read number in the upper 23 bits, the three 3-bit codes (columns c0, c0 + 1, c0 + 2) in the
// lower nine.  The read number names the entry while it is made and in the host checks; it is not stored (below).
#define JL_IX_READ_BITS 23u
#define JL_IX_MAX_READS (1ull << JL_IX_READ_BITS)   // windows with more reads get no index
JL_IX_FN uint32_t jl_ix_encode(uint32_t read, uint32_t a, uint32_t b, uint32_t c) { return (read << 9) | (a << 6) | (b << 3) | c; }
JL_IX_FN uint32_t jl_ix_read(uint32_t e) { return e >> 9; }
JL_IX_FN uint32_t jl_ix_code(uint32_t e, uint32_t j) { return (e >> (6u - 3u * j)) & 7u; }   // j = 0, 1, 2
// ---- the entry as it is stored: the low 16 bits — the nine code bits (a << 6) | (b << 3) | c, the upper seven zero.  Nothing reads
// a stored read number: the walk (index_stream) takes e & 0x1FF only, lists have no order, and no API hands entries out
// (jl_index_info gives counts).  So the 23 bits would be written by the build, kept in HBM and fetched on every run for nothing;
// without them a list is half the bytes and half the dependent round trips of its walk.
typedef uint16_t jl_ix_stored_t;
#define JL_IX_ENTRY_BYTES 2u
JL_IX_FN jl_ix_stored_t jl_ix_stored(uint32_t e) { return (jl_ix_stored_t)(e & 0x1FFu); }

// ---- bounds, all in ENTRIES.  A chunk is indexed while 4 E is at most half of its nine plane rows' bytes — the rule of the 4-byte
// entry, kept as it is (the sweep behind it is of that entry; a higher bound for the cheaper list is a change of its own): in bytes
// a stored list is now at most a quarter of the chunk's plane rows.  The window has an index while all its lists together hold at
// most 3 n_cols plane_stride / 8 entries.  (numerator / denominator: the sweep of profiles/ changes these two only)
#ifndef JL_IX_DENSITY_NUM
#define JL_IX_DENSITY_NUM 1u
#define JL_IX_DENSITY_DEN 2u
#endif
// most entries of an indexed chunk: 4 E <= 9 plane_stride NUM / DEN
JL_IX_FN uint64_t jl_ix_chunk_max_entries(uint64_t plane_stride) { return 9u * plane_stride * JL_IX_DENSITY_NUM / (4u * JL_IX_DENSITY_DEN); }
// a chunk's list begins on a multiple of four entries = 8 bytes (a lane loads four entries at once): its room in the buffer
JL_IX_FN uint64_t jl_ix_padded(uint64_t entries) { return (entries + 3u) & ~(uint64_t)3u; }
// most entries (padded) of a whole index: one per eight bytes of the matrix's planes.  While a chunk's bound is at most one entry
// per eight of its own plane bytes the plain chunks' bounds add up to no more than this, so this bound only limits the allocation when
// the density bound (JL_IX_DENSITY_NUM / DEN) is swept above a half; an index is REFUSED in practice only when no chunk is under its
// own bound.
JL_IX_FN uint64_t jl_ix_total_max_entries(uint64_t plane_stride, uint32_t n_cols) { return 3u * (uint64_t)n_cols * plane_stride / 8u; }
// what is allocated before the build, with no host round trip in the middle: the smaller of the two bounds
JL_IX_FN uint64_t jl_ix_alloc_entries(uint64_t plane_stride, uint32_t n_cols, uint32_t n_plain)
{
    const uint64_t by_chunk = (uint64_t)n_plain * jl_ix_padded(jl_ix_chunk_max_entries(plane_stride));
    const uint64_t by_total = jl_ix_padded(jl_ix_total_max_entries(plane_stride, n_cols));
    return (by_chunk < by_total ? by_chunk : by_total) + 4u;
}
// (in bytes x JL_IX_ENTRY_BYTES: what the entry buffer takes and jl_index_info.bytes reports; the benchmark's window: 28.2 MB)

// ---- the counting kernel's per-lane accumulators: one 64-bit word per column, a 9-bit field per code 0..6 (63 bits).  A lane
// takes four entries a round (one 8-byte load of stored entries), each adds one to one field of each column: a field holds at most
// 511, so a batch is at most 127 rounds (508), and the 64 lanes of a wave sum to at most 64 x 508 = 32512 < 2^16: two fields per DPP sum.
#define JL_IX_FIELD_BITS 9u
#define JL_IX_ROUND_ENTRIES 4u
#define JL_IX_FLUSH_ROUNDS 127u
#define JL_IX_BLOCK_LANES 256u
JL_IX_FN uint32_t jl_ix_field_max(void) { return (1u << JL_IX_FIELD_BITS) - 1u; }
// entries of a chunk that one workgroup walks without a flush in between: beyond it the flush edge is crossed
JL_IX_FN uint64_t jl_ix_flush_entries(void) { return (uint64_t)JL_IX_FLUSH_ROUNDS * JL_IX_ROUND_ENTRIES * JL_IX_BLOCK_LANES; }

// ---- the walk's depth: rounds a lane holds in registers, all their loads out before the first is consumed (kernels_pileup.hip
// index_stream).  With 8-byte rounds the depths are twice those of the 4-byte entry, for the same registers and the same bytes in
// flight per workgroup: 2 in the unfolded kernels (4 KB), 16 in the folded ones (32 KB).  A flush falls on whole batches of `depth`
// rounds, never above JL_IX_FLUSH_ROUNDS: 126 rounds (504 a field) at depth 2, 112 (448) at depth 16.
#ifndef JL_IX_DEPTH
#define JL_IX_DEPTH 2u
#endif
#ifndef JL_IX_FOLD_DEPTH
#define JL_IX_FOLD_DEPTH 16u
#endif
#define JL_IX_MAX_DEPTH 16u
JL_IX_FN constexpr uint32_t jl_ix_flush_rounds_at(uint32_t depth) { return JL_IX_FLUSH_ROUNDS / depth * depth; }

// ---- the record a build leaves in pinned host memory (jl_ctx::h_ix) and jl_msa_index_info hands out
#define JL_IX_NONE 0u
#define JL_IX_PENDING 1u
#define JL_IX_BUILT 2u
#define JL_IX_REFUSED 3u
