// kernels_hypermut.hip — per-read APOBEC hypermutation counters over the whole resident window and their exact test
// (jl_read_hypermut_async; docs/SPEC.md §26): for every read its G->A sites in the target context GRD and in the control contexts,
// and of each kind the mutated ones.  The context of a site is the READ's own two cells downstream, so the count is a stencil of
// three columns over the bit planes — a vertical sum as in kernels_readstats.hip, whose shape, bit-sliced counters and batch
// loader (read_walk.h) it shares.
// Shape (readstats_shape.h): a wave is a workgroup; lane l owns word 64 chunk + l of every plane row.  The segment [c0, c1) walks
// the columns t = c0 .. min(c1 + 2, n_cols) - 1 in batches of kBatch, the next batch in flight while this one is counted, and
// keeps the masks of the two columns behind t in registers: at column t it counts the site c = t - 2 (x at c, y at c + 1, z at t).
// The two columns at c1 and c1 + 1 are the HALO: loaded for context, their own sites belong to the next segment.  A site needs
// c + 2 < n_cols, which is t < n_cols: the last two columns of the window are never sites.  Per column, from the plane words:
//   base = ~p2    pur = base & ~p0 (A or G)    A = pur & ~p1    C = base & ~p1 & p0
//   site = [ref[c] == G] & valid & pur(c) & base(c + 1) & base(c + 2)
//   target = site & pur(c + 1) & ~C(c + 2)     control = site & ~target     mutated: & A(c)
// The four masks go into bit-sliced counters, emptied every 2^K - 1 columns into byte counters in LDS (a segment has at most 255
// sites); the epilogue hands the bytes on as kernels_readstats.hip does: as the segment's part for hypermut_combine_kernel, or by
// integer atomics into the zeroed output.  Both are exact and independent of launch shape and order.
// Addresses are formed from the sizes capi_hypermut.hip checked: a load reads plane row r < 3 n_cols at bytes [4 w, 4 w + 4) with
// w < ceil(n_reads / 32), within every accepted plane stride; ref is read at c < n_cols; what a word holds beyond n_reads is cut
// by jl_valid_bits.
#include "hypermut_test.h"
#include "jl_internal.h"
#include "planes.h"
#include "read_walk.h"
#include "readstats_shape.h"

namespace {

using namespace jl_read_walk;

// grid: x = segment * n_chunks + chunk
template <uint32_t K, bool ATOMIC>
__global__ __launch_bounds__(64) void hypermut_count_kernel(jl_hypermut_args a)
{
    __shared__ uint32_t s_acc[JL_HM_COUNTERS * kKindDwords];
    const uint32_t lane = threadIdx.x;
    const uint32_t chunk = blockIdx.x % a.n_chunks, seg = blockIdx.x / a.n_chunks;
    const uint32_t word = chunk * 64u + lane;
    const bool have = word < a.n_words;
    const uint32_t valid = have ? jl_valid_bits(a.n_reads, word) : 0u;
    const uint32_t c0 = seg * a.seg_cols, c1 = min(c0 + a.seg_cols, a.n_cols);   // (seg < n_segs: c0 < n_cols)
    const uint32_t ce = min(c1 + 2u, a.n_cols);                                  // the walk's end: the segment and its halo
    const uint8_t JL_AS1 *word0 = (const uint8_t JL_AS1 *)a.msa + 4ull * word;
    const uint8_t JL_AS1 *ref = (const uint8_t JL_AS1 *)a.ref;

    uint32_t *mine = s_acc + lane * kLaneDwords;
#pragma unroll
    for (uint32_t q = 0; q < JL_HM_COUNTERS; ++q)
#pragma unroll
        for (uint32_t g = 0; g < 8u; ++g) mine[q * kKindDwords + g] = 0u;

    sliced<K> cnt[JL_HM_COUNTERS];
#pragma unroll
    for (uint32_t q = 0; q < JL_HM_COUNTERS; ++q) cnt[q].clear();
    uint32_t pending = 0u;   // sites added since the last flush
    uint32_t pur2 = 0u, a2 = 0u;               // of column t - 2: purine (cut to the reads), A
    uint32_t base1 = 0u, pur1 = 0u, a1 = 0u;   // of column t - 1

    batch cur, nxt;
    cur.load(word0, a.plane_stride, c0, ce, have);
    for (uint32_t c = c0; c < ce; c += kBatch) {
        if (c + kBatch < ce) nxt.load(word0, a.plane_stride, c + kBatch, ce, have);   // in flight while this batch is counted
#pragma unroll
        for (uint32_t i = 0; i < kBatch; ++i) {
            const uint32_t t = c + i;
            if (t < ce) {   // (wave-uniform)
                const uint32_t p0 = cur.p[3u * i], p1 = cur.p[3u * i + 1u], p2 = cur.p[3u * i + 2u];
                const uint32_t base = ~p2, pur = base & ~p0;
                if (t >= c0 + 2u) {   // (wave-uniform) the site at t - 2, of this segment: c0 <= t - 2 < c1
                    const uint32_t on = (uint32_t)ref[t - 2u] == 2u ? 0xFFFFFFFFu : 0u;   // (wave-uniform)
                    const uint32_t site = on & pur2 & base1 & base;
                    const uint32_t target = site & pur1 & ~(~p1 & p0);
                    const uint32_t control = site & ~target;
                    cnt[JL_HM_TARGET_SITES].add(target);
                    cnt[JL_HM_TARGET_MUT].add(target & a2);
                    cnt[JL_HM_CONTROL_SITES].add(control);
                    cnt[JL_HM_CONTROL_MUT].add(control & a2);
                    if (++pending == (1u << K) - 1u) {
#pragma unroll
                        for (uint32_t q = 0; q < JL_HM_COUNTERS; ++q) cnt[q].flush(mine + q * kKindDwords);
                        pending = 0u;
                    }
                }
                pur2 = pur1, a2 = a1;
                base1 = base, pur1 = valid & pur, a1 = pur & ~p1;
            }
        }
        cur = nxt;
    }
#pragma unroll
    for (uint32_t q = 0; q < JL_HM_COUNTERS; ++q) cnt[q].flush(mine + q * kKindDwords);
    __syncthreads();

    const uint64_t read0 = (uint64_t)chunk * JL_RS_WG_READS;
    if (!ATOMIC) {
        // the segment's part: per kind the workgroup's 512 dwords of four byte counters, in read order, all of them
        uint32_t *part = a.part + ((uint64_t)seg * JL_HM_COUNTERS * a.n_chunks + chunk) * kQuads;
#pragma unroll 1
        for (uint32_t u = lane; u < JL_HM_COUNTERS * kQuads; u += 64u) {
            const uint32_t q = u / kQuads, w = u % kQuads;
            part[(uint64_t)q * a.n_chunks * kQuads + w] = s_acc[q * kKindDwords + (w >> 3) * kLaneDwords + (w & 7u)];
        }
    } else {
#pragma unroll 1
        for (uint32_t u = lane; u < JL_HM_COUNTERS * JL_RS_WG_READS; u += 64u) {
            const uint32_t q = u / JL_RS_WG_READS, r = u % JL_RS_WG_READS;
            const uint32_t v = (s_acc[q * kKindDwords + (r >> 5) * kLaneDwords + ((r >> 2) & 7u)] >> (8u * (r & 3u))) & 0xFFu;
            if (v && read0 + r < a.n_reads) atomicAdd(a.counts + (uint64_t)q * a.n_reads + read0 + r, v);
        }
    }
}

// grid: x = 256 dwords of four reads, y = kind.  Every entry of the output is written.
__global__ __launch_bounds__(256) void hypermut_combine_kernel(jl_hypermut_args a, uint32_t n_segs)
{
    const uint64_t quad = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t q = blockIdx.y;
    if (4u * quad >= a.n_reads) return;
    const uint64_t kind_stride = (uint64_t)a.n_chunks * kQuads;   // (quad < kind_stride: 4 quad < n_reads <= 2048 n_chunks)
    const uint32_t JL_AS1 *part = (const uint32_t JL_AS1 *)a.part + q * kind_stride + quad;
    uint32_t s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u;
    for (uint32_t seg = 0; seg < n_segs; ++seg) {
        const uint32_t v = __builtin_nontemporal_load(part + (uint64_t)seg * JL_HM_COUNTERS * kind_stride);
        s0 += v & 0xFFu, s1 += (v >> 8) & 0xFFu, s2 += (v >> 16) & 0xFFu, s3 += v >> 24;
    }
    uint32_t *out = a.counts + (uint64_t)q * a.n_reads + 4u * quad;
    const uint64_t left = a.n_reads - 4u * quad;
    out[0] = s0;
    if (left > 1u) out[1] = s1;
    if (left > 2u) out[2] = s2;
    if (left > 3u) out[3] = s3;
}

// one thread a read: the table of its four counters through the header's routine (docs/SPEC.md §26)
__global__ __launch_bounds__(256) void hypermut_test_kernel(const uint32_t *__restrict__ counts, uint64_t n, double *__restrict__ p,
                                                             double *__restrict__ lp)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double l;
    p[i] = jl_hypermut_p(counts[JL_HM_TARGET_MUT * n + i], counts[JL_HM_TARGET_SITES * n + i], counts[JL_HM_CONTROL_MUT * n + i],
                         counts[JL_HM_CONTROL_SITES * n + i], &l);
    lp[i] = l;
}

template <bool ATOMIC>
void launch_counting(const jl_hypermut_args &A, const jl_readstats_shape &shape, hipStream_t st)
{
    const dim3 grid(shape.n_chunks * shape.n_segs), block(64);
    switch (shape.k) {
    case 4: hipLaunchKernelGGL((hypermut_count_kernel<4, ATOMIC>), grid, block, 0, st, A); break;
    case 5: hipLaunchKernelGGL((hypermut_count_kernel<5, ATOMIC>), grid, block, 0, st, A); break;
    default: hipLaunchKernelGGL((hypermut_count_kernel<6, ATOMIC>), grid, block, 0, st, A); break;
    }
}

}  // namespace

// shape.k in 4 .. 6; a->counts zeroed when the shape combines by atomics, a->part of jl_hypermut_part_words(shape) words otherwise
void jl_launch_hypermut_counts(const jl_hypermut_args *a, const jl_readstats_shape *shape, hipStream_t st)
{
    jl_hypermut_args A = *a;
    A.n_chunks = shape->n_chunks, A.seg_cols = shape->seg_cols;
    if (shape->combine == JL_RS_COMBINE_ATOMIC) {
        launch_counting<true>(A, *shape, st);
        return;
    }
    launch_counting<false>(A, *shape, st);
    const uint64_t quads = (A.n_reads + 3u) / 4u;
    hipLaunchKernelGGL(hypermut_combine_kernel, dim3((uint32_t)((quads + 255u) / 256u), JL_HM_COUNTERS), dim3(256), 0, st, A, shape->n_segs);
}

size_t jl_hypermut_part_words(const jl_readstats_shape *shape)
{
    return (size_t)shape->n_segs * JL_HM_COUNTERS * shape->n_chunks * kQuads;
}

void jl_launch_hypermut_test(const uint32_t *counts, uint64_t n, double *p, double *lp, hipStream_t st)
{
    hipLaunchKernelGGL(hypermut_test_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, counts, n, p, lp);
}
