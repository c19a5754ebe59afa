// kernels_orf.hip — per-read reading-frame counters per span over the resident window (jl_read_orf_async; docs/SPEC.md §27): for
// every (span, read) its covered cells, its gap cells, the codons it reads in full, the stop codons among those that the reference
// does not have, and the first of them.  A stop is a pattern over the three columns of a codon ON THE SPAN'S OWN GRID, and spans
// overlap in different frames: a three-column stencil per span, on the walk of the per-read counters (read_walk.h), whose bit-sliced
// counters and batch loader it uses as they stand.
// Shape (orf_shape.h): a wave is a workgroup; lane l owns word 64 chunk + l of every plane row.  A workgroup walks one SEGMENT of
// one span — whole codons of it, at most 85 (255 columns, what a byte counter holds) — in batches of kBatch columns, the next batch
// in flight while this one is counted.  No segment needs a column outside its own: no halo.  Per column, from the plane words:
//   base = ~p2    T = base & p0 & p1    A = base & ~p0 & ~p1    G = base & p1 & ~p0    gap = p2 & ~p1 & ~p0
//   covered = valid & ~(p2 & p1)
// and at the third column of the codon at c:
//   read3 = base(c) & base(c + 1) & base(c + 2) & valid
//   stop  = T(c) & ((A(c + 1) & (A | G)(c + 2)) | (G(c + 1) & A(c + 2))) & valid & [the reference codon is no stop]  (wave-uniform)
// The four masks go into bit-sliced counters, emptied every floor((2^K - 1) / 3) codons into byte counters in LDS (covered and gap
// take three additions a codon).  The FIRST stop is bit-sliced too: fresh = stop & ~seen takes the codon's offset in the segment
// (0 .. 84, wave-uniform) into seven slices, by or-ing fresh into the slices of the offset's set bits; it is handed on as a fifth
// kind of byte, 0xFF for none.  The epilogue hands the bytes on as the segment's part; orf_combine_kernel sums the four counters of
// every (span, read) over the span's segments and takes first_stop from the lowest segment whose byte is not 0xFF: the segment's
// first codon plus the byte.  Exact and independent of launch shape and order.
// Addresses are formed from the sizes capi_orf.hip checked: a load reads plane row r < 3 n_cols (every segment lies within its
// span, every span within the window: col + 3 n_codons <= n_cols) at bytes [4 w, 4 w + 4) with w < ceil(n_reads / 32), within every
// accepted plane stride; ref is read at c < n_cols; the segment table at seg < n_segs (the grid is n_segs * n_chunks), the spans'
// first segments at g <= n_spans; what a word holds beyond n_reads is cut by jl_valid_bits.
#include "jl_internal.h"
#include "orf_shape.h"
#include "planes.h"
#include "read_walk.h"

namespace {

using namespace jl_read_walk;

constexpr uint32_t kKinds = JL_ORF_COUNTERS + 1u;   // the four counters, and the first stop's offset
constexpr uint32_t kNone = 0xFFu;

__device__ __forceinline__ bool is_stop_codon(uint32_t r0, uint32_t r1, uint32_t r2)   // TAA, TAG, TGA (codes 0 .. 3 = A C G T)
{
    return r0 == 3u && ((r1 == 0u && (r2 == 0u || r2 == 2u)) || (r1 == 2u && r2 == 0u));
}

// grid: x = segment * n_chunks + chunk
template <uint32_t K>
__global__ __launch_bounds__(64) void orf_count_kernel(jl_orf_args a)
{
    constexpr uint32_t kFlush = ((1u << K) - 1u) / 3u;   // codons between two flushes: three additions a codon
    __shared__ uint32_t s_acc[kKinds * kKindDwords];
    const uint32_t lane = threadIdx.x;
    const uint32_t chunk = blockIdx.x % a.n_chunks, seg = blockIdx.x / a.n_chunks;
    const uint32_t word = chunk * 64u + lane;
    const bool have = word < a.n_words;
    const uint32_t valid = have ? jl_valid_bits(a.n_reads, word) : 0u;
    const jl_orf_seg JL_AS1 *sg = (const jl_orf_seg JL_AS1 *)a.segs + seg;   // (seg < n_segs)
    const uint32_t c0 = sg->col, ce = c0 + 3u * sg->n_codons;               // (ce <= n_cols)
    const uint8_t JL_AS1 *word0 = (const uint8_t JL_AS1 *)a.msa + 4ull * word;
    const uint8_t JL_AS1 *ref = (const uint8_t JL_AS1 *)a.ref;

    uint32_t *mine = s_acc + lane * kLaneDwords;
#pragma unroll
    for (uint32_t q = 0; q < JL_ORF_COUNTERS; ++q)
#pragma unroll
        for (uint32_t g = 0; g < 8u; ++g) mine[q * kKindDwords + g] = 0u;

    sliced<K> cnt[JL_ORF_COUNTERS];
#pragma unroll
    for (uint32_t q = 0; q < JL_ORF_COUNTERS; ++q) cnt[q].clear();
    sliced<7> first;            // the offset of the first stop, where `seen`
    first.clear();
    uint32_t seen = 0u;
    uint32_t pending = 0u;      // codons added since the last flush
    uint32_t phase = 0u;        // the column of its codon that t is (wave-uniform)
    uint32_t codon = 0u;        // ... and that codon's offset in the segment
    uint32_t t0 = 0u, read = 0u;    // of the codon so far: T at its first column; base at every column (cut to the reads)
    uint32_t a1 = 0u, g1 = 0u;      // A, G at its second column

    batch cur, nxt;
    cur.load(word0, a.plane_stride, c0, ce, have);
    for (uint32_t c = c0; c < ce; c += kBatch) {
        if (c + kBatch < ce) nxt.load(word0, a.plane_stride, c + kBatch, ce, have);   // in flight while this batch is counted
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) {
            const uint32_t t = c + i;
            if (t < ce) {   // (wave-uniform)
                const uint32_t p0 = cur.p[3u * i], p1 = cur.p[3u * i + 1u], p2 = cur.p[3u * i + 2u];
                const uint32_t base = ~p2;
                const uint32_t isA = base & ~p0 & ~p1, isG = base & p1 & ~p0;
                cnt[JL_ORF_COVERED].add(valid & ~(p2 & p1));
                cnt[JL_ORF_GAP_CELLS].add(valid & p2 & ~p1 & ~p0);
                if (phase == 0u) {
                    t0 = base & p0 & p1, read = valid & base;
                    phase = 1u;
                } else if (phase == 1u) {
                    a1 = isA, g1 = isG, read &= base;
                    phase = 2u;
                } else {
                    const bool ref_stop = is_stop_codon(ref[t - 2u], ref[t - 1u], ref[t]);   // (wave-uniform; t - 2 >= c0)
                    const uint32_t stop = ref_stop ? 0u : valid & t0 & ((a1 & (isA | isG)) | (g1 & isA));
                    cnt[JL_ORF_CODONS_READ].add(read & base);
                    cnt[JL_ORF_STOPS].add(stop);
                    const uint32_t fresh = stop & ~seen;
                    seen |= stop;
#pragma unroll
                    for (uint32_t b = 0; b < 7u; ++b)
                        if ((codon >> b) & 1u) first.s[b] |= fresh;
                    ++codon;
                    phase = 0u;
                    if (++pending == kFlush) {
#pragma unroll
                        for (uint32_t q = 0; q < JL_ORF_COUNTERS; ++q) cnt[q].flush(mine + q * kKindDwords);
                        pending = 0u;
                    }
                }
            }
        }
        cur = nxt;
    }
#pragma unroll
    for (uint32_t q = 0; q < JL_ORF_COUNTERS; ++q) cnt[q].flush(mine + q * kKindDwords);
    // the fifth kind: the offset's byte where a stop was seen, 0xFF where none
#pragma unroll
    for (uint32_t g = 0; g < 8u; ++g) {
        const uint32_t hit = ((((seen >> (4u * g)) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu;
        mine[JL_ORF_COUNTERS * kKindDwords + g] = (first.bytes(g) & hit) | ~hit;
    }
    __syncthreads();

    // the segment's part: per kind the workgroup's 512 dwords of four bytes, in read order, all of them
    uint32_t *part = a.part + ((uint64_t)seg * kKinds * a.n_chunks + chunk) * kQuads;
#pragma unroll 1
    for (uint32_t u = lane; u < kKinds * kQuads; u += 64u) {
        const uint32_t q = u / kQuads, w = u % kQuads;
        part[(uint64_t)q * a.n_chunks * kQuads + w] = s_acc[q * kKindDwords + (w >> 3) * kLaneDwords + (w & 7u)];
    }
}

// grid: x = 256 dwords of four reads, y = span.  Every entry of the output is written.
__global__ __launch_bounds__(256) void orf_combine_kernel(jl_orf_args a)
{
    const uint64_t quad = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t g = blockIdx.y;
    if (4u * quad >= a.n_reads) return;
    const uint64_t kind_stride = (uint64_t)a.n_chunks * kQuads;   // (quad < kind_stride: 4 quad < n_reads <= 2048 n_chunks)
    const uint32_t s0 = a.span_seg0[g], s1 = a.span_seg0[g + 1u];  // (g < n_spans; s0 < s1 <= n_segs)
    uint32_t sum[JL_ORF_COUNTERS][4] = {};
    uint32_t fs[4] = {JL_ORF_NO_STOP, JL_ORF_NO_STOP, JL_ORF_NO_STOP, JL_ORF_NO_STOP};
    for (uint32_t seg = s0; seg < s1; ++seg) {
        const uint32_t JL_AS1 *part = (const uint32_t JL_AS1 *)a.part + (uint64_t)seg * kKinds * kind_stride + quad;
#pragma unroll
        for (uint32_t q = 0; q < JL_ORF_COUNTERS; ++q) {
            const uint32_t v = __builtin_nontemporal_load(part + q * kind_stride);
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) sum[q][j] += (v >> (8u * j)) & 0xFFu;
        }
        const uint32_t f = __builtin_nontemporal_load(part + JL_ORF_COUNTERS * kind_stride);
        const uint32_t at = a.segs[seg].first_codon;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t b = (f >> (8u * j)) & 0xFFu;
            if (fs[j] == JL_ORF_NO_STOP && b != kNone) fs[j] = at + b;   // (segments ascend within a span: the lowest wins)
        }
    }
    const uint64_t left = a.n_reads - 4u * quad;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        if (j < left) {
#pragma unroll
            for (uint32_t q = 0; q < JL_ORF_COUNTERS; ++q) a.counts[((uint64_t)q * a.n_spans + g) * a.n_reads + 4u * quad + j] = sum[q][j];
            a.first_stop[(uint64_t)g * a.n_reads + 4u * quad + j] = fs[j];
        }
    }
}

}  // namespace

// shape->k in 4 .. 6; a->part of jl_orf_part_words(shape) words; a->segs and a->span_seg0 the table of that shape
void jl_launch_orf_counts(const jl_orf_args *a, const jl_orf_shape *shape, hipStream_t st)
{
    jl_orf_args A = *a;
    A.n_chunks = shape->n_chunks, A.n_segs = shape->n_segs;
    const dim3 grid((uint32_t)shape->grid), block(64);
    switch (shape->k) {
    case 4: hipLaunchKernelGGL((orf_count_kernel<4>), grid, block, 0, st, A); break;
    case 5: hipLaunchKernelGGL((orf_count_kernel<5>), grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL((orf_count_kernel<6>), grid, block, 0, st, A); break;
    }
    const uint64_t quads = (A.n_reads + 3u) / 4u;
    hipLaunchKernelGGL(orf_combine_kernel, dim3((uint32_t)((quads + 255u) / 256u), A.n_spans), dim3(256), 0, st, A);
}

size_t jl_orf_part_words(const jl_orf_shape *shape)
{
    return (size_t)shape->n_segs * kKinds * shape->n_chunks * kQuads;
}
