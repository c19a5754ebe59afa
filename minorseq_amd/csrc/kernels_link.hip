// kernels_link.hip — do two called variants occur on the same molecules (jl_variant_linkage_async; docs/SPEC.md §15).
// A read is one bit position in every plane row, so "read i can be read at codon position p" and "read i carries variant v" are
// bit ROWS, and every count the stage reports is popcount(row_a & row_b) summed over the words of the rows: a bit-matrix product.
// Stage 1, link_rows_kernel.  A lane owns one word (32 reads) of one position: it loads the position's nine plane words ONCE,
//   known   = ~(plane 2 of the three columns), cut to n_reads in the last word        -> informative row p
//   carry_v = known & ~OR_b (codon bit-word b ^ broadcast(bit b of var_codon[v]))     -> carry row of every variant v of p
// and writes zeros into the words of a row behind the last read (rows are whole 128-byte lines), so neither the padding nor what
// an adopted matrix holds behind byte ceil(n / 8) of a plane row ever enters a row.
// Stage 2, link_product_kernel.  The rows stand one above the other, M = [informative rows; carry rows], R = P + V of them, and
// G = M Mt holds all three outputs: both = G[I, I], carry = G[C, I], joint = G[C, C].  G is symmetric, so only its upper triangle
// is computed, and MIRRORED ON STORE.  Shape: a workgroup of four waves owns a 16 x 16 block of G and a run of split_words words;
// a wave owns an 8 x 8 tile of it (JL_LINK_TILE) and a lane the words lane, lane + 64, ... of the run: per round it loads its
// word of the tile's 8 + 8 rows (a coalesced 256 bytes a row and wave) and ANDs and counts the 64 pairs into 64 registers — a loaded
// word serves eight pairs, two VALU operations (v_and, v_bcnt with its accumulating operand) a pair.  The wave tile below the
// diagonal of a diagonal block is skipped.  The 64 per-lane sums are added over the wave by kernels_pileup.hip's DPP ladder, lane
// 8 i + j keeps pair (i, j) and adds it to the zeroed outputs with integer atomics: the runs of a row (blockIdx.z) and the two
// halves of a symmetric output meet there, exact and independent of launch shape and order.
// Addresses are formed from sizes the host checked only (capi_link.hip); var_codon bytes are data.
#include "jl_internal.h"

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    // full 64-lane sum by DPP; the total lands in lane 63
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);  // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);  // row_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1,3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2,3
    return v;
}

// grid: x = runs of 256 words of a row, y = position
__global__ __launch_bounds__(256) void link_rows_kernel(jl_link_args a)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x, p = blockIdx.y;
    if (w >= a.row_words) return;
    const uint32_t JL_AS1 *var_first = (const uint32_t JL_AS1 *)a.var_first;
    const uint32_t JL_AS1 *var_codon = (const uint32_t JL_AS1 *)a.var_codon;
    uint32_t JL_AS1 *rows = (uint32_t JL_AS1 *)a.rows;
    uint32_t known = 0u, bits[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    if (w < a.n_words) {   // (4 n_words <= plane_stride: a multiple of 16 and >= ceil(n / 8))
        const uint8_t JL_AS1 *src = (const uint8_t JL_AS1 *)a.msa + 3ull * ((const uint32_t JL_AS1 *)a.pos_cols)[p] * a.plane_stride + 4ull * w;
        uint32_t r[9];
#pragma unroll
        for (uint32_t q = 0; q < 9u; ++q) r[q] = *(const uint32_t JL_AS1 *)(src + (uint64_t)q * a.plane_stride);
        known = ~(r[2] | r[5] | r[8]);
        const uint32_t tail = (uint32_t)(a.n_reads & 31u);
        if (w == a.n_words - 1u && tail) known &= (1u << tail) - 1u;
        // row 3 k + b = plane b of column k; codon bits 0, 1 = planes 0, 1 of column 2; 2, 3 of column 1; 4, 5 of column 0
        bits[0] = r[6], bits[1] = r[7], bits[2] = r[3], bits[3] = r[4], bits[4] = r[0], bits[5] = r[1];
    }
    rows[(uint64_t)p * a.row_words + w] = known;
    const uint32_t v_end = var_first[p + 1u];
    for (uint32_t v = var_first[p]; v < v_end; ++v) {   // (block-uniform)
        const uint32_t codon = var_codon[v];
        uint32_t mismatch = 0u;
#pragma unroll
        for (uint32_t b = 0; b < 6u; ++b) mismatch |= bits[b] ^ (0u - ((codon >> b) & 1u));
        rows[(uint64_t)(a.n_pos + v) * a.row_words + w] = known & ~mismatch;
    }
}

// grid: x, y = block column and block row of G (blocks below the diagonal leave at once), z = run of split_words words
__global__ __launch_bounds__(256, 4) void link_product_kernel(jl_link_args a)
{
    constexpr uint32_t T = JL_LINK_TILE;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (uniform, and known to be: row addresses in SGPRs)
    const uint32_t n_rows = a.n_pos + a.n_var;
    if (blockIdx.y > blockIdx.x) return;
    const uint32_t a0 = blockIdx.y * JL_LINK_BLOCK_TILE + (wave >> 1) * T, b0 = blockIdx.x * JL_LINK_BLOCK_TILE + (wave & 1u) * T;
    if (a0 > b0 || b0 >= n_rows) return;   // (wave-uniform; a0 <= b0 < n_rows from here on)
    const uint32_t JL_AS1 *rows = (const uint32_t JL_AS1 *)a.rows;
    const uint32_t JL_AS1 *ra[T], *rb[T];
#pragma unroll
    for (uint32_t i = 0; i < T; ++i) {   // a row beyond the last: the last one again, its sums are not stored
        ra[i] = rows + (uint64_t)min(a0 + i, n_rows - 1u) * a.row_words;
        rb[i] = rows + (uint64_t)min(b0 + i, n_rows - 1u) * a.row_words;
    }
    uint32_t acc[T][T];
#pragma unroll
    for (uint32_t i = 0; i < T; ++i)
#pragma unroll
        for (uint32_t j = 0; j < T; ++j) acc[i][j] = 0u;
    const uint32_t begin = blockIdx.z * a.split_words, end = min(begin + a.split_words, a.n_words);
#pragma clang loop vectorize(disable) unroll(disable)
    for (uint32_t w = begin + lane; w < end; w += 64u) {
        uint32_t x[T], y[T];
#pragma unroll
        for (uint32_t i = 0; i < T; ++i) x[i] = ra[i][w], y[i] = rb[i][w];
#pragma unroll
        for (uint32_t i = 0; i < T; ++i)
#pragma unroll
            for (uint32_t j = 0; j < T; ++j) acc[i][j] += (uint32_t)__builtin_popcount(x[i] & y[j]);
    }
    uint32_t mine = 0u;   // lane 8 i + j keeps pair (i, j)
#pragma unroll
    for (uint32_t i = 0; i < T; ++i)
#pragma unroll
        for (uint32_t j = 0; j < T; ++j) {
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)wave_sum(acc[i][j]), 63);
            if (lane == T * i + j) mine = total;
        }
    const uint32_t ga = a0 + lane / T, gb = b0 + lane % T, P = a.n_pos, V = a.n_var;
    if (gb >= n_rows || ga > gb || mine == 0u) return;   // (ga > gb: the lower half of a tile on the diagonal)
    if (gb < P) {
        atomicAdd(a.both + (uint64_t)ga * P + gb, mine);
        if (ga != gb) atomicAdd(a.both + (uint64_t)gb * P + ga, mine);
    } else if (ga < P) {
        atomicAdd(a.carry + (uint64_t)(gb - P) * P + ga, mine);
    } else {
        atomicAdd(a.joint + (uint64_t)(ga - P) * V + (gb - P), mine);
        if (ga != gb) atomicAdd(a.joint + (uint64_t)(gb - P) * V + (ga - P), mine);
    }
}

}  // namespace

// a->both, a->carry, a->joint zeroed; a->split_words and a->n_splits set by the caller (capi_link.hip)
void jl_launch_variant_linkage(const jl_link_args *a, hipStream_t st)
{
    hipLaunchKernelGGL(link_rows_kernel, dim3((a->row_words + 255u) / 256u, a->n_pos), dim3(256), 0, st, *a);
    const uint32_t blocks = (a->n_pos + a->n_var + JL_LINK_BLOCK_TILE - 1u) / JL_LINK_BLOCK_TILE;
    hipLaunchKernelGGL(link_product_kernel, dim3(blocks, blocks, a->n_splits), dim3(256), 0, st, *a);
}
