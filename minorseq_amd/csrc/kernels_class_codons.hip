// kernels_class_codons.hip — codon histograms of the resident matrix BY CLASS OF READS at chosen codon starts
// (jl_class_codons_async; docs/SPEC.md §24): the codon counterpart of kernels_class.hip, hist[class][position][64].
// A class is a bit mask in the plane-row layout (the rows of class_masks_kernel, jl_launch_class_masks).  Per position a SEED
// codon is chosen (the majority base of each of its three columns among the first reads the wave sees); per 32 reads
//   valid = no plane-2 bit in any of the three columns (all three codes < 4)
//   match = valid & the six low plane words equal the seed's bits
// and the seed's count of class k is popcount(match & mask k), in registers.  Only the reads of valid & ~match that some class
// of the pass holds go on one by one: codon from their six bits, class from their LABEL — compared with the pass's class range,
// never an index before that — and one integer atomic on hist[class][position][codon].  The table does not depend on the seed:
// a read counts once for its own codon either way, by the popcount when it is the seed's and by the atomic when it is not.
// Shape: a lane owns a POSITION, a workgroup of four waves a group of 64 positions and a segment of the reads; the grid is
// (group, segment, pass of at most 16 classes), the classes of a pass a template argument as in kernels_class.hip.  Per tile of
// 512 reads the nine plane rows of every position (three columns x three planes, wherever the columns lie) are staged through
// LDS in the padded row layout of plane_walk.h by coalesced 16-byte loads, four threads a row; wave w counts words 4 w .. 4 w + 3
// of the tile, each lane reading its nine rows back as ds_read_b128.  The loads of the next tile are in flight while this one is
// counted.  Positions behind the last one are staged as zeros and count nowhere (`live`).
#include <array>
#include <utility>

#include "jl_internal.h"
#include "plane_walk.h"

namespace {

using namespace jl_walk;

constexpr uint32_t kStarts = 64;                    // positions of a group: one a lane
constexpr uint32_t kWaves = 4;                      // waves of a workgroup: a quarter of a tile's words each
constexpr uint32_t kThreads = 64 * kWaves;
constexpr uint32_t kRows = 9u * kStarts;            // plane rows staged: nine a position
constexpr uint32_t kLoads = kRows * 4u / kThreads;  // 16-byte loads of a thread per tile
static_assert(kStarts == 64, "jl_class_codons_shape_for (plane_walk.h) groups the positions by 64");
static_assert(kLoads * kThreads == kRows * 4u && kWaves * 4u == kTileWords, "a tile is four 16-byte units a row, one a wave");

// grid: x = group of 64 positions, y = read segment of `seg_tiles` tiles, z = pass; NK = classes of a pass, from class
// a.k_first + 16 z on
template <uint32_t NK>
__global__ __launch_bounds__(kThreads) void class_codons_kernel(jl_class_codons_args a)
{
    __shared__ u32x4 s_rows[rows::slot(kRows)];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t p0 = blockIdx.x * kStarts, p = p0 + lane;
    const bool live = p < a.n_pos;
    const uint32_t k0 = a.k_first + blockIdx.z * 16u;
    const range seg = segment(a.n_reads, a.seg_tiles);
    const uint8_t JL_AS1 *planes = (const uint8_t JL_AS1 *)a.msa;
    const uint32_t JL_AS1 *mask = (const uint32_t JL_AS1 *)((const uint8_t JL_AS1 *)a.mask + (uint64_t)k0 * a.mask_stride);
    const uint64_t mask_words = a.mask_stride / 4u;

    // what this thread stages: unit u = tid + 256 i is bytes 16 (u & 3) .. of staged row u >> 2 = plane row 3 col + r % 9 of
    // position p0 + r / 9 (the host checked col + 2 < n_cols: the row exists); kNoRow: no such position
    constexpr uint64_t kNoRow = ~0ull;
    uint64_t src[kLoads];
#pragma unroll
    for (uint32_t i = 0; i < kLoads; ++i) {
        const uint32_t r = (tid + kThreads * i) >> 2, q = p0 + r / 9u;
        src[i] = kNoRow;
        if (q < a.n_pos) src[i] = (3ull * ((const uint32_t JL_AS1 *)a.col)[q] + r % 9u) * a.plane_stride + 16u * (tid & 3u);
    }
    u32x4 v[kLoads];
    auto load = [&](uint32_t t) {   // zero where the position or the bytes do not exist
        const uint64_t at = (uint64_t)t * kTileBytes;
#pragma unroll
        for (uint32_t i = 0; i < kLoads; ++i) {
            v[i] = u32x4{0u, 0u, 0u, 0u};
            if (src[i] != kNoRow && at + 16u * (tid & 3u) + 16u <= a.plane_stride)
                v[i] = __builtin_nontemporal_load((const u32x4 JL_AS1 *)(planes + src[i] + at));
        }
    };

    uint32_t cnt[NK];
#pragma unroll
    for (uint32_t k = 0; k < NK; ++k) cnt[k] = 0u;
    uint32_t seed = 0u, x[6] = {0u, 0u, 0u, 0u, 0u, 0u};   // x[2 c + b]: all ones where bit b of the seed's base c is set

    if (seg.t0 < seg.t1) load(seg.t0);
    for (uint32_t t = seg.t0; t < seg.t1; ++t) {
        __syncthreads();   // every wave has read the tile before
#pragma unroll
        for (uint32_t i = 0; i < kLoads; ++i) {
            const uint32_t u = tid + kThreads * i;
            s_rows[rows::slot(u >> 2) + (u & 3u)] = v[i];
        }
        __syncthreads();
        if (t + 1u < seg.t1) load(t + 1u);   // in flight while this tile is counted
        u32x4 pl[9];   // pl[3 c + b] = plane b of column col + c, this wave's four words
#pragma unroll
        for (uint32_t r = 0; r < 9u; ++r) pl[r] = s_rows[rows::slot(9u * lane + r) + wave];

        if (t == seg.t0) {   // the seed: per column the base most of these 128 reads show (a hint only)
            seed = 0u;
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) {
                uint32_t n[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t b0 = pl[3u * c][j], b1 = pl[3u * c + 1u][j], b2 = pl[3u * c + 2u][j];
                    n[0] += __popc(~(b0 | b1 | b2));
                    n[1] += __popc(b0 & ~(b1 | b2));
                    n[2] += __popc(b1 & ~(b0 | b2));
                    n[3] += __popc(b0 & b1 & ~b2);
                }
                uint32_t best = 0u, bv = n[0];
#pragma unroll
                for (uint32_t s = 1; s < 4u; ++s)
                    if (n[s] > bv) bv = n[s], best = s;
                x[2u * c] = (best & 1u) ? 0xFFFFFFFFu : 0u;
                x[2u * c + 1u] = (best & 2u) ? 0xFFFFFFFFu : 0u;
                seed = seed * 4u + best;
            }
        }

        const uint32_t JL_AS1 *mw = mask + (uint64_t)t * kTileWords + 4u * wave;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t a0 = pl[0][j], a1 = pl[1][j], c0 = pl[3][j], c1 = pl[4][j], e0 = pl[6][j], e1 = pl[7][j];
            const uint32_t valid = live ? ~(pl[2][j] | pl[5][j] | pl[8][j]) : 0u;
            const uint32_t match = valid & ~((a0 ^ x[0]) | (a1 ^ x[1]) | (c0 ^ x[2]) | (c1 ^ x[3]) | (e0 ^ x[4]) | (e1 ^ x[5]));
            uint32_t any = 0u;   // reads of the pass's classes: none at or behind n_reads (the mask rows are zero there)
#pragma unroll
            for (uint32_t k = 0; k < NK; ++k) {
                const uint32_t m = mw[(uint64_t)k * mask_words + j];   // wave-uniform
                cnt[k] += __popc(match & m);
                any |= m;
            }
            uint32_t dev = valid & ~match & any;
            while (dev) {
                const uint32_t bit = (uint32_t)__ffs((int)dev) - 1u;
                dev &= dev - 1u;
                const uint64_t i = 32ull * ((uint64_t)t * kTileWords + 4u * wave + j) + bit;
                if (i >= a.n_reads) continue;
                const uint32_t k = (uint32_t)((const uint16_t JL_AS1 *)a.label)[i] - k0;   // (below k0: wraps beyond NK)
                if (k >= NK) continue;
                const uint32_t codon = (((a0 >> bit) & 1u) | (((a1 >> bit) & 1u) << 1)) * 16u +
                                       (((c0 >> bit) & 1u) | (((c1 >> bit) & 1u) << 1)) * 4u +
                                       (((e0 >> bit) & 1u) | (((e1 >> bit) & 1u) << 1));
                atomicAdd(a.hist + ((uint64_t)(k0 + k) * a.n_pos + p) * 64u + codon, 1u);
            }
        }
    }

    if (live) {
#pragma unroll
        for (uint32_t k = 0; k < NK; ++k)
            if (cnt[k]) atomicAdd(a.hist + ((uint64_t)(k0 + k) * a.n_pos + p) * 64u + seed, cnt[k]);
    }
}

template <uint32_t NK>
void launch_counting(const jl_class_codons_args &A, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL(class_codons_kernel<NK>, grid, dim3(kThreads), 0, st, A);
}

// kCounting[n - 1]: the counting launch of a pass of n classes
using counting_fn = void (*)(const jl_class_codons_args &, dim3, hipStream_t);
template <size_t... I>
constexpr std::array<counting_fn, sizeof...(I)> counting_table(std::index_sequence<I...>)
{
    return {launch_counting<(uint32_t)I + 1u>...};
}
constexpr auto kCounting = counting_table(std::make_index_sequence<16>{});

}  // namespace

// ceil(n_classes / 16) passes of the counting under mask rows that are there already; a->hist is zero
void jl_launch_class_codons(const jl_class_codons_args *a, hipStream_t st)
{
    jl_class_codons_args A = *a;
    const uint32_t n_groups = (A.n_pos + kStarts - 1u) / kStarts;
    const uint32_t full = A.n_classes / 16u, rest = A.n_classes % 16u;
    if (!jl_walk_tiles(A.n_reads)) return;   // no read: the zeroed table is the answer
    const jl_walk_shape shape = jl_class_codons_shape_for(A.n_reads, A.n_pos, A.n_classes);
    A.seg_tiles = shape.seg_tiles;
    const uint32_t n_segs = shape.n_segs;
    A.k_first = 0u;
    if (full) kCounting[15](A, dim3(n_groups, n_segs, full), st);
    A.k_first = 16u * full;
    if (rest) kCounting[rest - 1u](A, dim3(n_groups, n_segs, 1), st);
}
