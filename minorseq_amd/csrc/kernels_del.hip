// kernels_del.hip — which whole codons the reads of the resident matrix have deleted (jl_codon_deletions_async; docs/SPEC.md §16).
// Every column c with c + 2 < n_cols is a possible codon start; per start four counts over the reads, from the three codes at
// c, c + 1, c + 2:  codon (all three a base), del3 (all three '-'), partial ('-' and bases mixed, no N, no uncovered cell) and
// span (no uncovered cell).  A read is one bit position in every plane row, so per 32 reads the four sets are bit words:
//   b2 of a column = its cells with code 4, 5 or 6;  b2 & b1 = uncovered (6);  b2 & b0 = N once the uncovered ones are out
//   span    = valid & ~(uncovered of c | of c + 1 | of c + 2)            valid: the bits of the word that are reads
//   clean   = span & ~(N of c | of c + 1 | of c + 2)                     every cell of such a read is a base or '-'
//   codon   = span & ~(b2 | b2 | b2)        del3 = clean & (b2 & b2 & b2)        partial = clean & ((b2 | b2 | b2) ^ (b2 & b2 & b2))
// about twenty VALU operations and four popcounts a word.
// Shape: the tile walk of plane_walk.h.  A lane owns a codon START; staged are the 198 plane rows of the group's 64 columns and
// of the HALO of two columns behind them, and a lane reads the nine rows of its three columns back.  The loads of the next tile
// are issued before the current one is counted.  A lane's four counters go out as 16 contiguous bytes.
#include "jl_internal.h"
#include "plane_walk.h"

namespace {

using namespace jl_walk;

constexpr uint32_t kStarts = 64;        // codon starts of a group: one a lane
constexpr uint32_t kRows = 3u * (kStarts + 2u);      // plane rows staged: the group's columns and the halo of two

// grid: x = group of 64 codon starts, y = read segment of `seg_tiles` tiles
__global__ __launch_bounds__(64) void codon_deletions_kernel(jl_del_args a)
{
    __shared__ u32x4 s_rows[rows::slot(kRows)];
    const uint32_t lane = threadIdx.x;
    const uint32_t col0 = blockIdx.x * kStarts, col = col0 + lane;
    const range seg = segment(a.n_reads, a.seg_tiles);
    const rows staged{3u * min(kStarts + 2u, a.n_cols - col0)};   // plane rows of this group and its halo that exist
    const uint8_t JL_AS1 *planes = (const uint8_t JL_AS1 *)a.msa + 3ull * col0 * a.plane_stride;

    uint32_t codon = 0u, del3 = 0u, partial = 0u, span = 0u;
    tile<kRows, rows> v;
    if (seg.t0 < seg.t1) v.load(staged, planes, a.plane_stride, seg.t0, lane);
    for (uint32_t t = seg.t0; t < seg.t1; ++t) {
        v.store(s_rows, lane);
        if (t + 1u < seg.t1) v.load(staged, planes, a.plane_stride, t + 1u, lane);   // in flight while this tile is counted
#pragma unroll 1
        for (uint32_t q = 0; q < kTileWords / 4u; ++q) {
            u32x4 p[9];   // p[3 k + b] = plane b of column col + k
#pragma unroll
            for (uint32_t r = 0; r < 9u; ++r) p[r] = s_rows[rows::slot(3u * lane + r) + q];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t valid = jl_valid_bits(a.n_reads, t * kTileWords + 4u * q + j);   // (wave-uniform)
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

// a->cnt zeroed, a->n_cols >= 3
void jl_launch_codon_deletions(const jl_del_args *a, hipStream_t st)
{
    jl_del_args A = *a;
    const uint32_t n_groups = (A.n_cols - 2u + kStarts - 1u) / kStarts;
    const jl_walk_shape shape = jl_walk_shape_for(A.n_reads, n_groups);
    A.seg_tiles = shape.seg_tiles;
    hipLaunchKernelGGL(codon_deletions_kernel, dim3(n_groups, shape.n_segs), dim3(64), 0, st, A);
}
