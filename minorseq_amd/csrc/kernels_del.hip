// kernels_del.hip — which whole codons the reads of the resident matrix have deleted (jl_codon_deletions_async; docs/SPEC.md §16).
// Every column c with c + 2 < n_cols is a possible codon start; per start four counts over the reads, from the three codes at
// c, c + 1, c + 2:  codon (all three a base), del3 (all three '-'), partial ('-' and bases mixed, no N, no uncovered cell) and
// span (no uncovered cell).  A read is one bit position in every plane row, so per 32 reads the four sets are bit words:
//   b2 of a column = its cells with code 4, 5 or 6;  b2 & b1 = uncovered (6);  b2 & b0 = N once the uncovered ones are out
//   span    = valid & ~(uncovered of c | of c + 1 | of c + 2)            valid: the bits of the word that are reads
//   clean   = span & ~(N of c | of c + 1 | of c + 2)                     every cell of such a read is a base or '-'
//   codon   = span & ~(b2 | b2 | b2)        del3 = clean & (b2 & b2 & b2)        partial = clean & ((b2 | b2 | b2) ^ (b2 & b2 & b2))
// about twenty VALU operations and four popcounts a word.
// Shape: kernels_class.hip's.  A lane owns a codon START (64 starts a wave, one wave a workgroup) and walks a segment of the
// reads; the grid is (group of 64 starts, read segment).  Per tile of 512 reads (64 bytes of every plane row) the 198 plane rows
// of the group's 64 columns and of the HALO of two columns behind them are staged through LDS by coalesced 16-byte loads — four
// lanes a row, sixteen rows a load instruction — and each lane reads the nine rows of its three columns back as ds_read_b128
// (rows padded to 80 bytes: lane l starts 60 l dwords on, conflict-free within the instruction's 16-lane groups).  The loads of
// the next tile are issued before the current one is counted.  A lane keeps its four counters in registers across the segment: no
// wave reduction; the counts are integers added to the zeroed table with integer atomics at the end, 16 contiguous bytes a lane:
// independent of order and of the launch shape.
// Addresses are formed from the sizes the host checked only (capi_del.hip): a load reads row r < 3 n_cols at bytes [at, at + 16)
// with at + 16 <= plane_stride.  What a tile holds beyond the plane row or the last column is zero in LDS; the bits of a word
// beyond n_reads — the padding, and whatever an adopted matrix holds there — are cut by `valid`.
#include "jl_internal.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kTileBytes = 64;     // bytes of a plane row a tile stages: 512 reads, 16 words
constexpr uint32_t kTileWords = kTileBytes / 4u;
constexpr uint32_t kRowDwords = 20;     // a staged row in LDS: 16 words + 4 of padding
constexpr uint32_t kStarts = 64;        // codon starts of a group: one a lane
constexpr uint32_t kRows = 3u * (kStarts + 2u);      // plane rows staged: the group's columns and the halo of two
constexpr uint32_t kLoads = (kRows + 15u) / 16u;     // load instructions a tile: sixteen rows each, the last one six

// 16 bytes of rows 16 i + (lane >> 2) of tile t, zero where the row or the bytes do not exist
__device__ __forceinline__ void load_tile(const jl_del_args &a, const uint8_t JL_AS1 *planes, uint32_t n_rows, uint32_t t, uint32_t lane,
                                          u32x4 (&v)[kLoads])
{
    const uint64_t at = (uint64_t)t * kTileBytes + 16u * (lane & 3u);
#pragma unroll
    for (uint32_t i = 0; i < kLoads; ++i) {
        const uint32_t row = 16u * i + (lane >> 2);
        v[i] = u32x4{0u, 0u, 0u, 0u};
        if (row < n_rows && at + 16u <= a.plane_stride)
            v[i] = __builtin_nontemporal_load((const u32x4 JL_AS1 *)(planes + (uint64_t)row * a.plane_stride + at));
    }
}

// grid: x = group of 64 codon starts, y = read segment of `seg_tiles` tiles
__global__ __launch_bounds__(64) void codon_deletions_kernel(jl_del_args a)
{
    __shared__ u32x4 s_rows[kRows * kRowDwords / 4u];
    const uint32_t lane = threadIdx.x;
    const uint32_t col0 = blockIdx.x * kStarts, col = col0 + lane;
    const uint32_t n_words = (uint32_t)((a.n_reads + 31u) / 32u);
    const uint32_t n_tiles = (n_words + kTileWords - 1u) / kTileWords;
    const uint32_t t0 = blockIdx.y * a.seg_tiles, t1 = min(t0 + a.seg_tiles, n_tiles);
    const uint32_t n_rows = 3u * min(kStarts + 2u, a.n_cols - col0);   // plane rows of this group and its halo that exist
    const uint8_t JL_AS1 *planes = (const uint8_t JL_AS1 *)a.msa + 3ull * col0 * a.plane_stride;

    uint32_t codon = 0u, del3 = 0u, partial = 0u, span = 0u;
    u32x4 v[kLoads];
    if (t0 < t1) load_tile(a, planes, n_rows, t0, lane, v);
    for (uint32_t t = t0; t < t1; ++t) {
        __syncthreads();   // the last tile has been read
#pragma unroll
        for (uint32_t i = 0; i < kLoads; ++i) {
            const uint32_t row = 16u * i + (lane >> 2);
            if (row < kRows) s_rows[row * (kRowDwords / 4u) + (lane & 3u)] = v[i];
        }
        __syncthreads();
        if (t + 1u < t1) load_tile(a, planes, n_rows, t + 1u, lane, v);   // in flight while this tile is counted
#pragma unroll 1
        for (uint32_t q = 0; q < kTileWords / 4u; ++q) {
            u32x4 p[9];   // p[3 k + b] = plane b of column col + k
#pragma unroll
            for (uint32_t r = 0; r < 9u; ++r) p[r] = s_rows[(3u * lane + r) * (kRowDwords / 4u) + q];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                // the reads of this word that exist (wave-uniform)
                const int64_t left = (int64_t)a.n_reads - 32ll * (int64_t)(t * kTileWords + 4u * q + j);
                const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : left > 0 ? (1u << (uint32_t)left) - 1u : 0u;
                const uint32_t x0 = p[0][j], x1 = p[1][j], x2 = p[2][j];
                const uint32_t y0 = p[3][j], y1 = p[4][j], y2 = p[5][j];
                const uint32_t z0 = p[6][j], z1 = p[7][j], z2 = p[8][j];
                const uint32_t any2 = x2 | y2 | z2, all2 = x2 & y2 & z2;
                const uint32_t in = valid & ~((x2 & x1) | (y2 & y1) | (z2 & z1));      // no uncovered cell
                const uint32_t clean = in & ~((x2 & x0) | (y2 & y0) | (z2 & z0));      // ... and no N: bases and '-' only
                codon += __popc(in & ~any2);
                del3 += __popc(clean & all2);
                partial += __popc(clean & (any2 ^ all2));
                span += __popc(in);
            }
        }
    }

    if ((uint64_t)col + 2u < a.n_cols) {
        uint32_t *out = a.cnt + (uint64_t)col * 4u;
        if (codon) atomicAdd(out + 0, codon);
        if (del3) atomicAdd(out + 1, del3);
        if (partial) atomicAdd(out + 2, partial);
        if (span) atomicAdd(out + 3, span);
    }
}

}  // namespace

// tiles a read segment walks: segments x groups fill the chip a few times over (kernels_class.hip's rule)
static uint32_t del_seg_tiles(uint32_t n_tiles, uint32_t n_groups)
{
    const uint32_t want_blocks = 4096u;   // 256 CUs x 8 one-wave workgroups, twice
    const uint32_t segs = std::max(1u, std::min(n_tiles, want_blocks / std::max(1u, n_groups)));
    const uint32_t tiles = (n_tiles + segs - 1u) / segs;
    return (tiles + 1u) & ~1u;   // whole 128-byte lines
}

// a->cnt zeroed, a->n_cols >= 3
void jl_launch_codon_deletions(const jl_del_args *a, hipStream_t st)
{
    jl_del_args A = *a;
    const uint32_t n_words = (uint32_t)((A.n_reads + 31u) / 32u);
    const uint32_t n_tiles = (n_words + kTileWords - 1u) / kTileWords;
    const uint32_t n_groups = (A.n_cols - 2u + kStarts - 1u) / kStarts;
    A.seg_tiles = del_seg_tiles(n_tiles, n_groups);
    const uint32_t n_segs = (n_tiles + A.seg_tiles - 1u) / A.seg_tiles;
    hipLaunchKernelGGL(codon_deletions_kernel, dim3(n_groups, n_segs), dim3(64), 0, st, A);
}
