// kernels_class.hip — column pileup of the resident matrix BY CLASS OF READS (jl_class_pileup_async; docs/SPEC.md §13).
// A read is one bit position in every plane row, so a class of reads is a BIT MASK in the plane-row layout and a per-class
// symbol count is popcount(symbol word & class mask) over the words the plain pileup streams:
//   class_masks_kernel    label[n_reads] -> one mask row per class (read i = bit i & 7 of byte i >> 3, as a plane row; every bit
//                         at or beyond n_reads clear, out to the end of the row) and class_reads[k]
//   class_pileup_kernel   counts[k][column][A C G T - N] of at most 16 classes a pass (blockIdx.z = pass; the classes of a pass
//                         are a template argument: their counters are registers)
// Shape of the counting: the tile walk of plane_walk.h — a lane owns a COLUMN, the grid is (column group, read segment, pass), the
// 192 plane rows of the wave's columns are staged per tile of 512 reads, loaded at the top of the iteration and stored at once.
// The class mask words are the same for all columns of the wave: wave-uniform loads, once per read word.  Per 32 reads the six
// symbol words come from the three plane words by the identities of kernels_pileup.hip (code 7 does not occur): T = b0 & b1,
// N = b0 & b2, uncovered = b1 & b2, C G - the remainders of b0 b1 b2, A what no plane has.  A lane keeps its 16 x 6 counters in
// registers across the segment: 12 VALU operations per class and word, which is what bounds the kernel.
// A label is data: it is compared with the class numbers a wave builds rows for and never indexes anything.
#include <array>
#include <utility>

#include "jl_internal.h"
#include "plane_walk.h"

namespace {

using namespace jl_walk;

constexpr uint32_t kMaskWaves = 4;      // waves of a masks workgroup: the same line of reads, different classes
constexpr uint32_t kRows = 192;         // plane rows of a wave's 64 columns

// grid: x = line of 1024 reads (128 bytes of every mask row), y = class chunk (classes beyond the grid's y: a loop)
__global__ __launch_bounds__(64 * kMaskWaves) void class_masks_kernel(jl_class_args a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * 1024u + lane;
    uint32_t lab[16];   // the labels of reads i0 + 64 q; a read that does not exist belongs to no class
#pragma unroll
    for (uint32_t q = 0; q < 16u; ++q) {
        const uint64_t i = i0 + 64u * q;
        lab[q] = i < a.n_reads ? (uint32_t)((const uint16_t JL_AS1 *)a.label)[i] : 0xFFFFFFFFu;
    }
    for (uint32_t k = blockIdx.y * kMaskWaves + wave; k < a.n_classes; k += gridDim.y * kMaskWaves) {
        uint64_t mine = 0;
        uint32_t members = 0;
#pragma unroll
        for (uint32_t q = 0; q < 16u; ++q) {
            const uint64_t m = __ballot(lab[q] == k);   // reads 64 q .. 64 q + 63 of the line: its q-th 8 bytes
            members += (uint32_t)__popcll(m);
            if (lane == q) mine = m;
        }
        if (lane < 16u) *(uint64_t JL_AS1 *)((uint8_t JL_AS1 *)a.mask + (uint64_t)k * a.mask_stride + (uint64_t)blockIdx.x * 128u + 8u * lane) = mine;
        if (lane == 0u && members) atomicAdd(a.class_reads + k, members);
    }
}

// grid: x = group of 64 columns, y = read segment of `seg_tiles` tiles, z = pass; NK = classes of a pass, from class
// a.k_first + 16 z on (the launcher: the full passes with NK = 16, what is left over with its own count)
template <uint32_t NK>
__global__ __launch_bounds__(64) void class_pileup_kernel(jl_class_args a)
{
    __shared__ u32x4 s_rows[rows::slot(kRows)];
    const uint32_t lane = threadIdx.x;
    const uint32_t col0 = blockIdx.x * 64u, col = col0 + lane;
    const uint32_t k0 = a.k_first + blockIdx.z * 16u;
    const range seg = segment(a.n_reads, a.seg_tiles);
    const rows staged{3u * min(64u, a.n_cols - col0)};   // plane rows of this group that exist
    const uint8_t JL_AS1 *planes = (const uint8_t JL_AS1 *)a.msa + 3ull * col0 * a.plane_stride;
    // the mask rows have a stride of their own, whole 128-byte lines of n_reads whatever the planes' is: every word of every
    // tile exists in them, and the words behind the last read are zero — a tile needs no end of its own
    const uint32_t JL_AS1 *mask = (const uint32_t JL_AS1 *)((const uint8_t JL_AS1 *)a.mask + (uint64_t)k0 * a.mask_stride);
    const uint64_t mask_words = a.mask_stride / 4u;

    uint32_t cnt[NK][6];
#pragma unroll
    for (uint32_t k = 0; k < NK; ++k)
#pragma unroll
        for (uint32_t s = 0; s < 6u; ++s) cnt[k][s] = 0u;

    for (uint32_t t = seg.t0; t < seg.t1; ++t) {
        tile<kRows, rows> v;   // what lies beyond a plane row or the last column is zero, and no class has a read there
        v.load(staged, planes, a.plane_stride, t, lane);
        v.store(s_rows, lane);
        const uint32_t JL_AS1 *mw = mask + (uint64_t)t * kTileWords;
#pragma unroll 1
        for (uint32_t q = 0; q < kTileWords / 4u; ++q, mw += 4) {
            const u32x4 p0 = s_rows[rows::slot(3u * lane + 0u) + q];
            const u32x4 p1 = s_rows[rows::slot(3u * lane + 1u) + q];
            const u32x4 p2 = s_rows[rows::slot(3u * lane + 2u) + q];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t b0 = p0[j], b1 = p1[j], b2 = p2[j];
                uint32_t sym[6];
                sym[3] = b0 & b1;            // T
                sym[5] = b0 & b2;            // N
                sym[1] = b0 & ~(b1 | b2);    // C
                sym[2] = b1 & ~(b0 | b2);    // G
                sym[4] = b2 & ~(b0 | b1);    // -
                sym[0] = ~(b0 | b1 | b2);    // A (b1 & b2: no read there, counted nowhere)
#pragma unroll
                for (uint32_t k = 0; k < NK; ++k) {
                    const uint32_t m = mw[(uint64_t)k * mask_words + j];   // wave-uniform
#pragma unroll
                    for (uint32_t s = 0; s < 6u; ++s) cnt[k][s] += __popc(sym[s] & m);
                }
            }
        }
    }

    if (col < a.n_cols) {
#pragma unroll
        for (uint32_t k = 0; k < NK; ++k) {
            uint32_t *out = a.counts + ((uint64_t)(k0 + k) * a.n_cols + col) * 6u;
#pragma unroll
            for (uint32_t s = 0; s < 6u; ++s)
                if (cnt[k][s]) atomicAdd(out + s, cnt[k][s]);
        }
    }
}

template <uint32_t NK>
void launch_counting(const jl_class_args &A, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL(class_pileup_kernel<NK>, grid, dim3(64), 0, st, A);
}

// kCounting[n - 1]: the counting launch of a pass of n classes
using counting_fn = void (*)(const jl_class_args &, dim3, hipStream_t);
template <size_t... I>
constexpr std::array<counting_fn, sizeof...(I)> counting_table(std::index_sequence<I...>)
{
    return {launch_counting<(uint32_t)I + 1u>...};
}
constexpr auto kCounting = counting_table(std::make_index_sequence<16>{});

}  // namespace

// masks and class_reads from the labels (the per-class codon tables of kernels_class_codons.hip count under the same rows);
// a->class_reads is zero, a->msa, a->counts and the columns are not looked at
void jl_launch_class_masks(const jl_class_args *a, hipStream_t st)
{
    const uint32_t n_lines = (uint32_t)((a->n_reads + 1023u) / 1024u);
    const uint32_t class_chunks = (a->n_classes + kMaskWaves - 1u) / kMaskWaves;
    hipLaunchKernelGGL(class_masks_kernel, dim3(n_lines, class_chunks), dim3(64 * kMaskWaves), 0, st, *a);
}

// the masks, then ceil(n_classes / 16) passes of the counting; a->counts and a->class_reads are zero
void jl_launch_class_pileup(const jl_class_args *a, hipStream_t st)
{
    jl_class_args A = *a;
    jl_launch_class_masks(&A, st);
    const uint32_t n_groups = (A.n_cols + 63u) / 64u;
    const jl_walk_shape shape = jl_walk_shape_for(A.n_reads, n_groups);
    A.seg_tiles = shape.seg_tiles;
    const uint32_t full = A.n_classes / 16u, rest = A.n_classes % 16u;
    A.k_first = 0u;
    if (full) kCounting[15](A, dim3(n_groups, shape.n_segs, full), st);
    A.k_first = 16u * full;
    if (rest) kCounting[rest - 1u](A, dim3(n_groups, shape.n_segs, 1), st);
}
