// read_walk.h — what the per-read walks over the bit planes share (kernels_readstats.hip, docs/SPEC.md §20; kernels_hypermut.hip,
// §26): the bit-sliced counter of a lane's 32 reads, the batch of columns a lane keeps in flight, and the sizes of the byte
// counters in LDS that both kernels hand on.  A wave is a workgroup; lane l owns word 64 chunk + l of every plane row
// (readstats_shape.h).  Private to libjuliet_hip.so; device code only.
#pragma once
#include "jl_internal.h"
#include "readstats_shape.h"

namespace jl_read_walk {

constexpr uint32_t kBatch = 8;                   // columns loaded together: 24 dwords a lane in flight
constexpr uint32_t kLaneDwords = 9;              // a lane's byte counters of one kind in LDS: 8 dwords + 1 of padding (no bank twice)
constexpr uint32_t kKindDwords = 64u * kLaneDwords;
constexpr uint32_t kQuads = JL_RS_WG_READS / 4u; // dwords of four byte counters a workgroup hands on per kind

template <uint32_t K>
struct sliced {
    uint32_t s[K];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) s[j] = 0u;
    }
    // + 1 for the reads of m: a ripple of half adders (no carry leaves slice K - 1 within 2^K - 1 additions)
    __device__ __forceinline__ void add(uint32_t m)
    {
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) {
            const uint32_t carry = s[j] & m;
            s[j] ^= m;
            m = carry;
        }
    }
    // the counts of reads 4 g .. 4 g + 3 as four bytes (bit i of a nibble times 0x00204081 lands on bit 8 i, nothing collides)
    __device__ __forceinline__ uint32_t bytes(uint32_t g) const
    {
        uint32_t v = 0u;
#pragma unroll
        for (uint32_t j = 0; j < K; ++j) v |= ((((s[j] >> (4u * g)) & 0xFu) * 0x00204081u) & 0x01010101u) << j;
        return v;
    }
    __device__ __forceinline__ void flush(uint32_t *acc)   // acc: the lane's kLaneDwords of this kind
    {
#pragma unroll
        for (uint32_t g = 0; g < 8u; ++g) acc[g] += bytes(g);
        clear();
    }
};

struct batch {
    uint32_t p[3u * kBatch];
    // columns c .. c + kBatch - 1 of the walk ending at c1; zero where the column or the lane's word does not exist
    __device__ __forceinline__ void load(const uint8_t JL_AS1 *word0, uint64_t plane_stride, uint32_t c, uint32_t c1, bool have)
    {
#pragma unroll
        for (uint32_t i = 0; i < 3u * kBatch; ++i) {
            p[i] = 0u;
            if (have && c + i / 3u < c1)
                p[i] = __builtin_nontemporal_load((const uint32_t JL_AS1 *)(word0 + (3ull * c + i) * plane_stride));
        }
    }
};

}  // namespace jl_read_walk
