// kernels_readstats.hip — per-read counters over the whole resident window (jl_read_stats_async; docs/SPEC.md §20): for every read
// its bases, gaps, masked cells, the bases in compared columns and the mismatches among those.  A read is one bit position in every
// plane row, so a per-read count is a vertical sum over 3 n_cols plane rows: lanes own read words and walk columns, where every
// other counting kernel has lanes own columns and popcount.
// Shape (readstats_shape.h): a wave is a workgroup; lane l owns word 64 chunk + l of every plane row, so each load instruction is
// 256 contiguous bytes of one row (global-typed, non-temporal: the matrix is read once).  Columns come in batches of kBatch, the
// next batch in flight while this one is counted.  Per column, from the three plane words and the wave-uniform compare code b:
//   base = valid & ~p2      gap = valid & p2 & ~p1 & ~p0      masked = valid & p2 & ~p1 & p0      (p2 & p1: uncovered, nowhere)
//   compared = base where b < 4      mismatch = compared & ((p0 ^ -b0) | (p1 ^ -b1))
// Each mask is added into a bit-sliced counter: word j holds bit j of the count of each of the word's 32 reads, a mask goes in by
// a ripple of K half adders.  No popcount and no atomic per cell.  After 2^K - 1 columns (and at the segment's end) the slices are
// emptied: four reads' K-bit counts are spread into the four bytes of a dword and added to the lane's own byte counters in LDS
// (a segment has at most 255 columns).  The epilogue reads the bytes back in read order and either stores them as the segment's
// part (combined by read_stats_combine_kernel) or adds them to the zeroed output with integer atomics, 256 contiguous bytes an
// instruction.  Both are exact and independent of launch shape and order.
// Addresses are formed from the sizes capi_readstats.hip checked: a load reads plane row r < 3 n_cols at bytes [4 w, 4 w + 4) with
// w < ceil(n_reads / 32), which is within every accepted plane stride (a multiple of 16, at least ceil(n_reads / 8)); what a word
// holds beyond n_reads is cut by jl_valid_bits.
#include "jl_internal.h"
#include "planes.h"
#include "read_walk.h"
#include "readstats_shape.h"

namespace {

using namespace jl_read_walk;   // sliced<K>, batch and the sizes of the byte counters in LDS (read_walk.h: shared with kernels_hypermut.hip)

// grid: x = segment * n_chunks + chunk
template <uint32_t K, bool ATOMIC>
__global__ __launch_bounds__(64) void read_stats_kernel(jl_readstats_args a)
{
    __shared__ uint32_t s_acc[JL_READ_STATS * kKindDwords];
    const uint32_t lane = threadIdx.x;
    const uint32_t chunk = blockIdx.x % a.n_chunks, seg = blockIdx.x / a.n_chunks;
    const uint32_t word = chunk * 64u + lane;
    const bool have = word < a.n_words;
    const uint32_t valid = have ? jl_valid_bits(a.n_reads, word) : 0u;
    const uint32_t c0 = seg * a.seg_cols, c1 = min(c0 + a.seg_cols, a.n_cols);   // (seg < n_segs: c0 < n_cols)
    const uint8_t JL_AS1 *word0 = (const uint8_t JL_AS1 *)a.msa + 4ull * word;
    const uint8_t JL_AS1 *cmp = (const uint8_t JL_AS1 *)a.compare;

    uint32_t *mine = s_acc + lane * kLaneDwords;
#pragma unroll
    for (uint32_t q = 0; q < JL_READ_STATS; ++q)
#pragma unroll
        for (uint32_t g = 0; g < 8u; ++g) mine[q * kKindDwords + g] = 0u;

    sliced<K> cnt[JL_READ_STATS];
#pragma unroll
    for (uint32_t q = 0; q < JL_READ_STATS; ++q) cnt[q].clear();
    uint32_t pending = 0u;   // columns added since the last flush

    batch cur, nxt;
    cur.load(word0, a.plane_stride, c0, c1, have);
    for (uint32_t c = c0; c < c1; c += kBatch) {
        if (c + kBatch < c1) nxt.load(word0, a.plane_stride, c + kBatch, c1, have);   // in flight while this batch is counted
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) {
            if (c + i < c1) {   // (wave-uniform)
                const uint32_t b = cmp ? (uint32_t)cmp[c + i] : 4u;   // (wave-uniform)
                const uint32_t on = b < 4u ? 0xFFFFFFFFu : 0u, b0 = 0u - (b & 1u), b1 = 0u - ((b >> 1) & 1u);
                const uint32_t p0 = cur.p[3u * i], p1 = cur.p[3u * i + 1u], p2 = cur.p[3u * i + 2u];
                const uint32_t base = valid & ~p2, low = valid & p2 & ~p1;
                const uint32_t compared = base & on;
                cnt[JL_READ_BASES].add(base);
                cnt[JL_READ_GAPS].add(low & ~p0);
                cnt[JL_READ_MASKED].add(low & p0);
                cnt[JL_READ_COMPARED].add(compared);
                cnt[JL_READ_MISMATCHES].add(compared & ((p0 ^ b0) | (p1 ^ b1)));
                if (++pending == (1u << K) - 1u) {
#pragma unroll
                    for (uint32_t q = 0; q < JL_READ_STATS; ++q) cnt[q].flush(mine + q * kKindDwords);
                    pending = 0u;
                }
            }
        }
        cur = nxt;
    }
#pragma unroll
    for (uint32_t q = 0; q < JL_READ_STATS; ++q) cnt[q].flush(mine + q * kKindDwords);
    __syncthreads();

    const uint64_t read0 = (uint64_t)chunk * JL_RS_WG_READS;
    if (!ATOMIC) {
        // the segment's part: per kind the workgroup's 512 dwords of four byte counters, in read order, all of them
        uint32_t *part = a.part + ((uint64_t)seg * JL_READ_STATS * a.n_chunks + chunk) * kQuads;
#pragma unroll 1
        for (uint32_t u = lane; u < JL_READ_STATS * kQuads; u += 64u) {
            const uint32_t q = u / kQuads, w = u % kQuads;
            part[(uint64_t)q * a.n_chunks * kQuads + w] = s_acc[q * kKindDwords + (w >> 3) * kLaneDwords + (w & 7u)];
        }
    } else {
#pragma unroll 1
        for (uint32_t u = lane; u < JL_READ_STATS * JL_RS_WG_READS; u += 64u) {
            const uint32_t q = u / JL_RS_WG_READS, r = u % JL_RS_WG_READS;
            const uint32_t v = (s_acc[q * kKindDwords + (r >> 5) * kLaneDwords + ((r >> 2) & 7u)] >> (8u * (r & 3u))) & 0xFFu;
            if (v && read0 + r < a.n_reads) atomicAdd(a.stats + (uint64_t)q * a.n_reads + read0 + r, v);
        }
    }
}

// grid: x = 256 dwords of four reads, y = kind.  Every entry of the output is written.
__global__ __launch_bounds__(256) void read_stats_combine_kernel(jl_readstats_args a, uint32_t n_segs)
{
    const uint64_t quad = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t q = blockIdx.y;
    if (4u * quad >= a.n_reads) return;
    const uint64_t kind_stride = (uint64_t)a.n_chunks * kQuads;   // (quad < kind_stride: 4 quad < n_reads <= 2048 n_chunks)
    const uint32_t JL_AS1 *part = (const uint32_t JL_AS1 *)a.part + q * kind_stride + quad;
    uint32_t s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u;
    for (uint32_t seg = 0; seg < n_segs; ++seg) {
        const uint32_t v = __builtin_nontemporal_load(part + (uint64_t)seg * JL_READ_STATS * kind_stride);
        s0 += v & 0xFFu, s1 += (v >> 8) & 0xFFu, s2 += (v >> 16) & 0xFFu, s3 += v >> 24;
    }
    uint32_t *out = a.stats + (uint64_t)q * a.n_reads + 4u * quad;
    const uint64_t left = a.n_reads - 4u * quad;
    out[0] = s0;
    if (left > 1u) out[1] = s1;
    if (left > 2u) out[2] = s2;
    if (left > 3u) out[3] = s3;
}

template <bool ATOMIC>
void launch_counting(const jl_readstats_args &A, const jl_readstats_shape &shape, hipStream_t st)
{
    const dim3 grid(shape.n_chunks * shape.n_segs), block(64);
    switch (shape.k) {
    case 4: hipLaunchKernelGGL((read_stats_kernel<4, ATOMIC>), grid, block, 0, st, A); break;
    case 5: hipLaunchKernelGGL((read_stats_kernel<5, ATOMIC>), grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL((read_stats_kernel<6, ATOMIC>), grid, block, 0, st, A); break;
    }
}

}  // namespace

// shape.k in 4 .. 6; a->stats zeroed when the shape combines by atomics, a->part of jl_readstats_part_words(shape) words otherwise
void jl_launch_read_stats(const jl_readstats_args *a, const jl_readstats_shape *shape, hipStream_t st)
{
    jl_readstats_args A = *a;
    A.n_chunks = shape->n_chunks, A.seg_cols = shape->seg_cols;
    if (shape->combine == JL_RS_COMBINE_ATOMIC) {
        launch_counting<true>(A, *shape, st);
        return;
    }
    launch_counting<false>(A, *shape, st);
    const uint64_t quads = (A.n_reads + 3u) / 4u;
    hipLaunchKernelGGL(read_stats_combine_kernel, dim3((uint32_t)((quads + 255u) / 256u), JL_READ_STATS), dim3(256), 0, st, A, shape->n_segs);
}

size_t jl_readstats_part_words(const jl_readstats_shape *shape)
{
    return (size_t)shape->n_segs * JL_READ_STATS * shape->n_chunks * kQuads;
}
