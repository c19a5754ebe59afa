// plane_walk.h — the tile walk of the kernels that count over whole plane rows: the per-class pileup (kernels_class.hip), the
// codon deletions (kernels_del.hip) and the junction span (kernels_ins.hip).  Private to libjuliet_hip.so.
// Shape.  A lane owns a column (or codon start, or junction), a wave is a workgroup and walks a SEGMENT of the reads; the grid is
// (group of 64, read segment).  Per tile of 512 reads (64 bytes of every plane row) the plane rows of the group, with the halo its
// kernel needs, are staged through LDS by coalesced 16-byte non-temporal loads — four lanes a row, sixteen rows a load
// instruction, no lane pulls bytes out of a line of its own — and each lane reads its own rows back as ds_read_b128.  Counters
// stay in registers across the segment (no wave reduction) and are added to the zeroed output with integer atomics at the end:
// independent of order and of the launch shape.
// LDS layouts, both conflict-free within ds_read_b128's 16-lane groups: a row padded to 80 bytes where a lane reads three
// consecutive rows per column (`rows`: lane l starts 60 l dwords on); a column's two rows next to each other in 36 dwords where
// it reads two (kernels_ins.hip: lane l starts 36 l dwords on).
// Addresses are formed from the sizes the host checked only (capi_class.hip, capi_del.hip, capi_ins.hip): a load reads a plane
// row r < 3 n_cols — the kernel's layout says which, and that it exists — at bytes [at, at + 16) with at + 16 <= plane_stride.
// What a tile holds beyond the plane row (the caller's stride may end inside the tile) or beyond the last column is zero in LDS;
// the bits of a word beyond n_reads are cut by jl_valid_bits (planes.h), or by mask rows that have none there.
// Two schedules are written on the same pieces.  Deletions and span load tile t + 1 after store()'s second barrier, in flight
// while tile t is counted.  The class pileup loads at the top of the iteration and stores at once: the prefetch would keep 48
// more VGPRs live beside its 96 counters, a speed change that wants a measurement of its own.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "planes.h"

// ---- host: the launch shape.  A workgroup walks `seg_tiles` tiles; the grid's y is n_segs.  n_reads > 0.
struct jl_walk_shape {
    uint32_t seg_tiles, n_segs;
};

// segments x groups fill the chip a few times over, a segment being whole 128-byte lines of every row (an even count of tiles)
static inline jl_walk_shape jl_walk_shape_for(uint64_t n_reads, uint32_t n_groups)
{
    const uint32_t want_blocks = 4096u;   // 256 CUs x 8 one-wave workgroups, twice
    const uint32_t n_tiles = jl_walk_tiles(n_reads);
    const uint32_t segs = std::max(1u, std::min(n_tiles, want_blocks / std::max(1u, n_groups)));
    jl_walk_shape s;
    s.seg_tiles = ((n_tiles + segs - 1u) / segs + 1u) & ~1u;
    s.n_segs = (n_tiles + s.seg_tiles - 1u) / s.seg_tiles;
    return s;
}

// the class-codon kernel's shape (kernels_class_codons.hip: groups of 64 positions, ceil(n_classes / 16) passes): segments x groups x
// passes fill the chip twice over, 256 CUs x 3 workgroups (46 KB of LDS each).  n_reads > 0.
static inline jl_walk_shape jl_class_codons_shape_for(uint64_t n_reads, uint32_t n_pos, uint32_t n_classes)
{
    const uint32_t n_groups = (n_pos + 63u) / 64u, full = n_classes / 16u;
    const uint32_t n_tiles = jl_walk_tiles(n_reads);
    const uint32_t segs = std::max(1u, std::min(n_tiles, 1536u / std::max(1u, n_groups * std::max(1u, full))));
    jl_walk_shape s;
    s.seg_tiles = (n_tiles + segs - 1u) / segs;
    s.n_segs = (n_tiles + s.seg_tiles - 1u) / s.seg_tiles;
    return s;
}

#if defined(__HIPCC__)
#include "jl_internal.h"

namespace jl_walk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kTileBytes = 64;     // bytes of a plane row a tile stages: 512 reads, 16 words
constexpr uint32_t kTileWords = kTileBytes / 4u;

// the tiles [t0, t1) of this workgroup's segment (blockIdx.y)
struct range {
    uint32_t t0, t1;
};
__device__ __forceinline__ range segment(uint64_t n_reads, uint32_t seg_tiles)
{
    const uint32_t t0 = blockIdx.y * seg_tiles;
    return range{t0, min(t0 + seg_tiles, jl_walk_tiles(n_reads))};
}

// A LAYOUT says, of staged row r: exists(r); plane_row(r), its plane row counted from the `planes` handed to load(); slot(r), its
// first 16-byte unit in LDS (four follow each other: a tile's 64 bytes).  This one: consecutive plane rows, the first n_rows exist.
struct rows {
    static constexpr uint32_t kRowDwords = 20;   // a staged row in LDS: 16 words + 4 of padding
    uint32_t n_rows;
    __device__ __forceinline__ bool exists(uint32_t r) const { return r < n_rows; }
    __device__ __forceinline__ uint64_t plane_row(uint32_t r) const { return r; }
    __device__ __forceinline__ static constexpr uint32_t slot(uint32_t r) { return r * (kRowDwords / 4u); }
};

// one tile of ROWS staged rows in registers: instruction i holds 16 bytes of rows 16 i .. 16 i + 15, four lanes a row
template <uint32_t ROWS, class LAYOUT>
struct tile {
    static constexpr uint32_t kLoads = (ROWS + 15u) / 16u;
    u32x4 v[kLoads];

    // tile t of the rows; zero where the row or the bytes do not exist.  `planes` is typed as global memory (JL_AS1): no flat loads
    __device__ __forceinline__ void load(const LAYOUT &l, const uint8_t JL_AS1 *planes, uint64_t plane_stride, uint32_t t, uint32_t lane)
    {
        const uint64_t at = (uint64_t)t * kTileBytes + 16u * (lane & 3u);
#pragma unroll
        for (uint32_t i = 0; i < kLoads; ++i) {
            const uint32_t r = 16u * i + (lane >> 2);
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (l.exists(r) && at + 16u <= plane_stride)
                v[i] = __builtin_nontemporal_load((const u32x4 JL_AS1 *)(planes + l.plane_row(r) * plane_stride + at));
        }
    }

    // into LDS, once every lane has read the tile before; visible to all on return
    __device__ __forceinline__ void store(u32x4 *lds, uint32_t lane) const
    {
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kLoads; ++i) {
            const uint32_t r = 16u * i + (lane >> 2);
            if (ROWS % 16u == 0u || r < ROWS) lds[LAYOUT::slot(r) + (lane & 3u)] = v[i];
        }
        __syncthreads();
    }
};

}  // namespace jl_walk
#endif
