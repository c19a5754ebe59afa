// kernels_recomb.hip — which reads are recombinants of two reported haplotypes (jl_phase_recombinants_async; docs/SPEC.md §23).
// The walk is hap_walk.h's: one wave a workgroup, runs of 64 reads, a lane a haplotype, the mismatch word per position.
// What is this kernel's own is ORDER.  Where the rescue keeps a bit and the nearest call a counter, this keeps `alive`, the reads that
// have not yet disagreed with the lane's haplotype, and where a bit of it dies at position p it records p BIT-SLICED: 13 words
// first[0..12] a read word, bit i of first[b] = bit b of the position at which read i first disagreed.  p is wave-uniform and the
// walk is hierarchical, so the slices are paid where they change: p = 64 t + 4 g + q with q a compile-time value, so
//   bits 0, 1   one OR of (alive & mismatch) per set bit of q (4 a group of four positions)
//   bits 2..5   once a group: the reads that died in it (alive before & ~alive after), ANDed with a scalar mask per bit of g
//   bits 6..12  once a tile, the same with the bits of t
// and once a chunk the reads still alive take n_pos itself, "never disagreed" — which is why there are 13 slices: 4096 must be
// representable.  About 16 VALU operations per position, word and lane where the rescue has 13.
// Per read the answer is hap_walk.h's sliced_verdict over the LARGEST first-mismatch index, 13 slices.  A haplotype slot h >= n_hap
// enters at 0 and the empty set is {0, no tie}: a tie flagged at 0 never shows, because a recombinant has P >= 1 and S >= 1
// (P + S >= n_pos with P < n_pos gives S >= 1; S == n_pos would make P == n_pos, so S < n_pos and P >= 1) and only a recombinant
// reports its ties.
// TWO PASSES, one function: the suffix of a read is its prefix over the positions in descending order, so the host hands over the
// positions and the packed pattern a second time, reversed, and pass 1 runs the code of pass 0 on them.  A pass ends in three
// numbers a lane (P or S, its tie, its id for the lane's read); the 2 x (13 + 1) + 2 x (13 + 1 + 10) words of slices and verdicts
// are alive in one pass only.  Sharing one pass over the staged tiles would keep both directions' 152 words at once — and the
// descending direction needs the LAST mismatch of an ascending walk, an overwrite of all 13 slices where this is an OR.
// parent_reads [n_hap][2] goes through an LDS histogram of the same shape; left, right, prefix and suffix leave by ordinary vector
// stores.  Addresses are formed from sizes the host checked only (capi_recomb.hip); pattern bytes are data.
#include "hap_walk.h"

namespace {

using namespace jl_hap;

constexpr uint32_t kSlices = 13;      // bits of a first-mismatch index: 0 .. 4096

typedef sliced_verdict<kSlices, true> verdict;   // best: the largest first-mismatch index in the set (0: nobody)

// where the reads of the two words first disagree with the lane's haplotype
struct first_mismatch {
    uint32_t alive[2];             // the reads that have not yet disagreed
    uint32_t first[2][kSlices];    // ... and where the others did first, sliced
    uint32_t in_tile[2], in_group[2];   // alive as the tile, the group began
    __device__ __forceinline__ void tile_begins() { in_tile[0] = alive[0], in_tile[1] = alive[1]; }
    __device__ __forceinline__ void group_begins() { in_group[0] = alive[0], in_group[1] = alive[1]; }
    template <class Q>
    __device__ __forceinline__ void operator()(uint32_t, Q, uint32_t j, uint32_t mismatch)
    {
        if (Q::value & 1u) first[j][0] |= alive[j] & mismatch;
        if (Q::value & 2u) first[j][1] |= alive[j] & mismatch;
        alive[j] &= ~mismatch;
    }
    __device__ __forceinline__ void group_ends(uint32_t g)
    {
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
            const uint32_t died = in_group[j] & ~alive[j];
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b) first[j][2u + b] |= died & (0u - ((g >> b) & 1u));
        }
    }
    __device__ __forceinline__ void tile_ends(uint32_t t)
    {
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
            const uint32_t died = in_tile[j] & ~alive[j];
#pragma unroll
            for (uint32_t b = 0; b < 7u; ++b) first[j][6u + b] |= died & (0u - ((t >> b) & 1u));
        }
    }
};

// what one direction says of the read of this lane
struct side {
    uint32_t len;   // P_i or S_i
    uint32_t tie;   // 1: two or more haplotypes attain it
    uint32_t id;    // the haplotype that attains it (valid where tie is 0)
};

// One direction over run `run`: the positions in the order of pos_cols, the pattern as pat4 packs it.  With COUNT, `informative`
// takes k_i of the lane's read in.
template <bool COUNT>
__device__ __forceinline__ side walk(const jl_recomb_args &a, uint32_t dir, uint32_t *s_pos, uint32_t run, uint32_t &informative)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t n_chunks = a.hap_pad / 64u;
    const table t = {(const uint8_t JL_AS1 *)a.msa, a.plane_stride, (const uint32_t JL_AS1 *)a.pos_cols[dir], (const uint32_t JL_AS1 *)a.pat4[dir], a.n_pos, a.hap_pad};
    verdict v[2];
    v[0].empty_set();
    v[1].empty_set();
    for (uint32_t c = 0; c < n_chunks; ++c) {
        first_mismatch f;
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
            f.alive[j] = 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t k = 0; k < kSlices; ++k) f.first[j][k] = 0u;
        }
        f = walk_chunk<COUNT>(t, s_pos, run, c, lane, informative, f);
        // the chunk's set: one haplotype a lane, at its first mismatch (never: n_pos; a slot beyond the last haplotype: 0)
        const uint32_t present = 64u * c + lane < a.n_hap ? 0xFFFFFFFFu : 0u;
#pragma unroll
        for (uint32_t j = 0; j < 2u; ++j) {
            verdict one;
            one.empty_set();
#pragma unroll
            for (uint32_t k = 0; k < kSlices; ++k) one.best[k] = (f.first[j][k] | (f.alive[j] & (0u - ((a.n_pos >> k) & 1u)))) & present;
#pragma unroll
            for (uint32_t b = 6; b < 10u; ++b) one.id[b] = id_slice(64u * c, b);
            v[j].join(one);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 2u; ++j) {
#pragma unroll
        for (uint32_t b = 0; b < 6u; ++b) v[j].id[b] = id_slice(lane, b);
        ladder(v[j]);
    }
    // expand (hap_walk.h): lane l answers for read 64 run + l = bit l & 31 of word l >> 5
    const uint32_t bit = lane & 31u, hi = lane >> 5;
    side s = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < kSlices; ++k) s.len |= (((hi ? v[1].best[k] : v[0].best[k]) >> bit) & 1u) << k;
#pragma unroll
    for (uint32_t b = 0; b < 10u; ++b) s.id |= (((hi ? v[1].id[b] : v[0].id[b]) >> bit) & 1u) << b;
    s.tie = ((hi ? v[1].tie : v[0].tie) >> bit) & 1u;
    return s;
}

// grid: x = one-wave workgroups, each walking the runs x, x + gridDim.x, ...; dynamic LDS: 2 n_hap words of histogram
__global__ __launch_bounds__(64) void phase_recombinants_kernel(jl_recomb_args a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_pos[kTilePos * kPosWords];
    extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];   // [n_hap][2]
    const uint32_t lane = threadIdx.x;
    const uint32_t n_hist = 2u * a.n_hap;
    clear(s_hist, n_hist, lane);
    uint32_t n_recombinant = 0, n_ambiguous = 0, n_whole = 0, n_none = 0, n_uninformative = 0;   // wave-uniform

    for (uint32_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
        uint32_t informative = 0;   // k_i of read 64 run + lane
        const side pre = walk<true>(a, 0, s_pos, run, informative);
        const side suf = walk<false>(a, 1, s_pos, run, informative);
        const uint64_t i = 64ull * run + lane;
        const bool exists = i < a.n_reads;
        uint32_t left, right;
        if (informative < a.min_positions) left = right = (uint32_t)JL_RESCUE_UNINFORMATIVE;
        else if (pre.len == a.n_pos) left = right = (uint32_t)JL_RECOMB_WHOLE;
        else if (pre.len + suf.len < a.n_pos) left = right = (uint32_t)JL_RESCUE_NONE;
        else {
            left = pre.tie ? (uint32_t)JL_RESCUE_AMBIGUOUS : pre.id;
            right = suf.tie ? (uint32_t)JL_RESCUE_AMBIGUOUS : suf.id;
        }
        const bool recombinant = exists && left < a.n_hap && right < a.n_hap;   // both parents unique: the histogram's cells exist
        const bool one_sided = exists && !recombinant && (left < a.n_hap || right < a.n_hap || left == (uint32_t)JL_RESCUE_AMBIGUOUS);
        if (exists) {
            ((uint16_t JL_AS1 *)a.left)[i] = (uint16_t)left;
            ((uint16_t JL_AS1 *)a.right)[i] = (uint16_t)right;
            ((uint16_t JL_AS1 *)a.prefix)[i] = (uint16_t)pre.len;
            ((uint16_t JL_AS1 *)a.suffix)[i] = (uint16_t)suf.len;
        }
        if (recombinant) {
            atomicAdd(&s_hist[2u * left], 1u);
            atomicAdd(&s_hist[2u * right + 1u], 1u);
        }
        n_recombinant += votes(recombinant);
        n_ambiguous += votes(one_sided);
        n_whole += votes(exists && left == (uint32_t)JL_RECOMB_WHOLE);
        n_none += votes(exists && left == (uint32_t)JL_RESCUE_NONE);
        n_uninformative += votes(exists && left == (uint32_t)JL_RESCUE_UNINFORMATIVE);
    }
    const uint32_t n[5] = {n_recombinant, n_ambiguous, n_whole, n_none, n_uninformative};
    flush(s_hist, n_hist, a.parent_reads, n, a.tally, lane);
}

}  // namespace

// a->parent_reads [n_hap][2] and a->tally [5] zeroed
void jl_launch_phase_recombinants(const jl_recomb_args *a, hipStream_t st)
{
    const size_t hist_bytes = (size_t)a->n_hap * 2u * sizeof(uint32_t);   // <= JL_RECOMB_HIST_WORDS words: 5.5 KiB
    hipLaunchKernelGGL(phase_recombinants_kernel, dim3(jl_hap_walk_blocks(a->n_runs)), dim3(64), hist_bytes, st, *a);
}
